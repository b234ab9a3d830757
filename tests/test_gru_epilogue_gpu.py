"""The fused GRU-gate and addend epilogue of the convolutions, and the 7x7 convolution at stride 1, one launch at a time against fp64.

um_conv2d_gru_fwd / um_conv2d_gru_add_fwd (conv.hip: conv_epilogue_pass, the GATE and ADD branches of store_rows, the side-tensor
preloading) are otherwise checked for values only through the whole refinement block (test_nhwc_update_block_matches_module), which
reaches the row-window kernel at exactly three full tiles.  Here every launch of the table in tests/gru_epilogue_util.py -- ragged last
tiles, several images with a ragged tile each, rows and columns shorter than the taps, a grid that is no multiple of the 8 XCDs, both
sides of conv_pick's 256-pixel threshold, a z | r boundary inside a tile -- gets inputs made from the reference (never another launch's
output), runs alone under the launch census, and is held to the project's gate for um_conv2d_ex outputs, 3e-6 x max(1, max|pre|): every
gate map is 1-Lipschitz in the pre-activation.  What a launch must NOT touch is compared bitwise with a snapshot: the other columns and
the zero row of the planes buffer it reads and writes (one 512-wide buffer, as in the block), the r half of z_out, the state it only
reads, addend, z and weights.  tests/test_gru_epilogue_cpu.py shows that six mutants of the reference would fail this gate.

um_conv7_fwd at stride 1 (the motion encoder's flow branch: pack7_kernel<8>, K = 448) against conv2d in fp64 under the stem's gate,
4e-6 x max(1, max|want|).  Every launch prints one record line; profiles/gru_epilogue.txt is that output on an MI355X."""
import pytest
import torch

from tests import gru_epilogue_util as gu
from unimatch_amd import _abi
from unimatch_amd.ops import HipOps

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = -12345.0
CONV_IDS = ('conv_patch', 'conv_rows', 'conv_generic')


@pytest.fixture(scope='module')
def ops():
    return HipOps('exact')


def rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def err(a, b):
    d = (a.double().cpu() - b.double().cpu()).abs()
    return d.max().item(), d.mean().item()


def census(lib, fn):
    """fn() with the launch census on -> (result, {variant: launches})."""
    lib.um_census_enable(1)
    try:
        out = fn()
    finally:
        counts = _abi.census(lib)
        lib.um_census_enable(0)
    return out, counts


def only(counts, *names):
    """The census id among ``names`` that counted; asserts that exactly one launch was counted among them."""
    hit = [n for n in names if counts[n]]
    assert len(hit) == 1 and counts[hit[0]] == 1, {n: counts[n] for n in names}
    return hit[0]


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16 if t.dtype == torch.float16 else t.dtype)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def planes_view(buf, rows, ld):
    return buf.view(torch.float16).view(2, rows + 1, ld)


def planes_untouched_outside(buf, snapshot, rows, ld, coff, c):
    """Every column but [coff, coff + c) of rows 0 .. rows - 1, and the whole zero row, bitwise as in the snapshot (both planes)."""
    now, was = bits(planes_view(buf, rows, ld)).clone(), bits(planes_view(snapshot, rows, ld)).clone()
    now[:, :rows, coff:coff + c] = 0
    was[:, :rows, coff:coff + c] = 0
    return torch.equal(now, was)


def run_launch(ops, case, gate, form):
    """One launch of the table -> worst error of its outputs; everything else is asserted here."""
    tag, b, hh, ww, c, _, ks = case
    ref = gu.reference(case, gate, form)
    lay, rows = ref['lay'], ref['rows']
    ld, coff = lay['ld'], lay['p_coff']
    tol = gu.value_gate(ref['pre'])
    G = ops.planes_buffer(rows, ld)
    ops.nhwc_gate(0, ref['buf'].to(DEV), G, ld, 0, rows, ld)
    wplanes = ops.conv_weight_planes_from(ref['weight'].to(DEV))
    wb = (wplanes, ref['bias'].to(DEV))
    h = ref['h'].to(DEV)
    addend = None if ref['addend'] is None else ref['addend'].to(DEV)
    snap = dict(G=G.clone(), w=wplanes[0].clone(), bias=wb[1].clone())
    src, outp, geom, pad = (G, ld, lay['a_coff'], lay['cin']), (G, ld, coff), (b, hh, ww), (ks[0] // 2, ks[1] // 2)
    if gate == 1:
        z_out = torch.full((rows, 2 * c), SENTINEL, dtype=torch.float32, device=DEV)
        _, counts = census(ops.lib, lambda: ops.conv_gru(1, src, geom, wb, ks, pad, h, outp, z_out=z_out, addend=addend))
    else:
        # z as the block hands it over: the z half of a [rows, 2C] tensor whose r half the launch must not read
        z = torch.full((rows, 2 * c), float('nan'), dtype=torch.float32, device=DEV)
        z[:, :c] = ref['z32'].to(DEV)
        zsnap = z.clone()
        hidden_out = torch.full((rows, c), SENTINEL, dtype=torch.float32, device=DEV) if form == 'addend+hidden_out' else None
        _, counts = census(ops.lib, lambda: ops.conv_gru(2, src, geom, wb, ks, pad, h, outp, z=z, addend=addend, hidden_out=hidden_out))
    torch.cuda.synchronize()
    kind, nt = gu.family(case, gate)
    assert only(counts, *CONV_IDS) == 'conv_' + kind, (tag, gate, form, counts)
    got_planes = planes_view(G, rows, ld).float().sum(0)[:rows, coff:coff + c]
    if gate == 1:
        e_z, e_p = err(z_out[:, :c], ref['z'])[0], err(got_planes, ref['rh'])[0]
        worst = max(e_z, e_p)
        gu.record(tag, gate, form, f'{kind} NT={nt}', worst, tol)
        assert e_z < tol and e_p < tol, (tag, gate, form, e_z, e_p, tol)
        # DESIGN.md, "Memory contract": gate 1 never writes the r half of z_out
        assert torch.equal(z_out[:, c:], torch.full((rows, c), SENTINEL, dtype=torch.float32, device=DEV)), (tag, form)
        assert same_bits(h, ref['h'].to(DEV)), (tag, form)
    else:
        state = hidden_out if hidden_out is not None else h
        e_h, e_p = err(state, ref['new'])[0], err(got_planes, ref['planes'])[0]
        worst = max(e_h, e_p)
        gu.record(tag, gate, form, f'{kind} NT={nt}', worst, tol)
        assert e_h < tol and e_p < tol, (tag, gate, form, e_h, e_p, tol)
        assert (got_planes - state).abs().max().item() < 1e-6, (tag, form)            # the bound of test_conv_ex_offsets_and_gates
        if hidden_out is not None:
            assert same_bits(h, ref['h'].to(DEV)), (tag, form)
        assert same_bits(z, zsnap), (tag, form)
    assert planes_untouched_outside(G, snap['G'], rows, ld, coff, c), (tag, gate, form)
    assert torch.equal(wplanes[0], snap['w']) and same_bits(wb[1], snap['bias']), (tag, gate, form)
    if addend is not None:
        assert same_bits(addend, ref['addend'].to(DEV)), (tag, gate, form)
    return worst


@pytest.mark.parametrize('gate', [1, 2])
@pytest.mark.parametrize('case', gu.CASES_128, ids=[c[0] for c in gu.CASES_128])
def test_gate_launch_matches_fp64(ops, case, gate):
    """C = 128 in the block's own operand layouts: plain (um_conv2d_gru_fwd, state updated in place), with the hoisted addend
    (um_conv2d_gru_add_fwd; gate 2 in place) and, gate 2, with the new state in ``hidden_out``."""
    for form in gu.FORMS[gate]:
        run_launch(ops, case, gate, form)


@pytest.mark.parametrize('gate', [1, 2])
@pytest.mark.parametrize('case', gu.CASES_SMALL, ids=[c[0] for c in gu.CASES_SMALL])
def test_gate_launch_off_product_channels(ops, case, gate):
    """C = 64 / 36 on 64 input channels: legal by the C ABI's argument checks, no product shape.  Gate 1 is one 128-wide tile with the
    z | r boundary in the middle of the tile (and, at cout = 72, dropped columns); gate 2 is NT = 2, the generic kernel even for 1x5."""
    for form in gu.FORMS[gate]:
        run_launch(ops, case, gate, form)


# ------------------------------------------------------------------ um_conv7_fwd at stride 1
def run_conv7(ops, image, weight, bias, cout):
    """bias + ReLU, fp32 and planes out of the same launch at non-zero column offsets of wider buffers -> (fp32 part, planes part as hi + lo);
    the guard columns and the planes' zero row are asserted bitwise untouched."""
    b, _, h, w = image.shape
    rows = b * h * w
    o_ld, o_coff, p_ld, p_coff = cout + 32, 16, cout + 64, 24
    f32 = torch.full((rows, o_ld), SENTINEL, dtype=torch.float32, device=DEV)
    dst = ops.planes_buffer(rows, p_ld)
    ops.nhwc_gate(0, rnd(31, rows, p_ld).to(DEV), dst, p_ld, 0, rows, p_ld)
    snap = dst.clone()
    _, counts = census(ops.lib, lambda: ops.conv7(image, weight, bias, 1, 1, out=(f32, o_ld, o_coff), outp=(dst, p_ld, p_coff)))
    torch.cuda.synchronize()
    assert only(counts, *CONV_IDS) == 'conv_generic', counts
    guard = torch.cat([f32[:, :o_coff], f32[:, o_coff + cout:]], 1)
    assert torch.equal(guard, torch.full_like(guard, SENTINEL))
    assert planes_untouched_outside(dst, snap, rows, p_ld, p_coff, cout)
    return f32[:, o_coff:o_coff + cout], planes_view(dst, rows, p_ld).float().sum(0)[:rows, p_coff:p_coff + cout]


@pytest.mark.parametrize('case', gu.CONV7_CASES, ids=[f'{s[0]}x{s[1]}x{s[2]}-c{ch}-n{co}' for s, ch, co in gu.CONV7_CASES])
def test_conv7_stride1_matches_fp64(ops, case):
    shape, ch, cout = case
    image, weight, bias = gu.conv7_inputs(shape, ch, cout)
    want = gu.conv7_reference(image, weight, bias)
    tol = gu.CONV7_REL * max(1.0, want.abs().max().item())
    got, got_planes = run_conv7(ops, image.to(DEV), weight.to(DEV), bias.to(DEV), cout)
    e_f, e_p = err(got, want)[0], err(got_planes, want)[0]
    print(f'CONV7-STRIDE1 | {shape[0]}x{shape[1]}x{shape[2]} | channels {ch} | cout {cout} | worst {max(e_f, e_p):.3e} | gate {tol:.3e}')
    assert e_f < tol and e_p < tol, (case, e_f, e_p, tol)


def test_conv7_weight_planes_follow_the_tensor(ops):
    """The packed 7x7 weight planes are cached by tensor identity: two weights of one shape, used one after the other and again, and
    temporaries that die between the calls (the allocator hands the next one the same address), each give their own result."""
    shape, ch, cout = (2, 9, 11), 2, 128
    image, w_a, bias = gu.conv7_inputs(shape, ch, cout)
    w_b = gu.conv7_inputs(shape, ch, cout, seed=1)[1]
    want_a, want_b = gu.conv7_reference(image, w_a, bias), gu.conv7_reference(image, w_b, bias)
    assert (want_a - want_b).abs().max().item() > 1.0
    img, bs, wa, wb = image.to(DEV), bias.to(DEV), w_a.to(DEV), w_b.to(DEV)
    for weight, want in ((wa, want_a), (wb, want_b), (wa, want_a)):
        got, _ = run_conv7(ops, img, weight, bs, cout)
        assert err(got, want)[0] < gu.CONV7_REL * max(1.0, want.abs().max().item())
    del wa, wb
    for seed in (2, 3, 4):
        w_t = gu.conv7_inputs(shape, ch, cout, seed=seed)[1]
        want = gu.conv7_reference(image, w_t, bias)
        got, _ = run_conv7(ops, img, w_t.to(DEV), bs, cout)
        assert err(got, want)[0] < gu.CONV7_REL * max(1.0, want.abs().max().item()), seed
