"""Every kernel-selection threshold from both sides, against fp64.

Each hot entry point picks a kernel instantiation, or a path inside one kernel, by a host-side rule on the call's geometry.  The rows
below put the smallest geometry that reaches it on each side of every such rule, run the entry point, assert WHICH side it ran on
(launch census where an id exists, the exported plan / part-count functions otherwise, plain arithmetic on the arguments where the rule
is nothing else -- helpers and citations in tests/dispatch_boundaries.py), and compare with the fp64 reference of the operation under
the gate the existing fp64 test of the same kernel applies:

  attention 5e-5 x max(1, |want|max) (1e-4 x for the mask-dominance probe); merged layer 5e-5; FFN 3e-5 (k | v epilogue: mean 2e-6,
  planes mean 4e-6); local softmaxes 2e-4; cost volumes 1e-4 x max; plane sweep 2e-4 x max (statistics: 2e-4 x their scale; arg-max:
  at most 1 % of the pixels off by more than 1e-6); convolutions 3e-6 x max (on-load and entry kernels 4e-6 x max, statistics feeding the
  norm 3e-5); norm 2e-5.  No new tolerance.

Thresholds that depend on the CU count are searched for with the plan functions on the device at hand; a side that is not found is a
failure.  Every case prints one DISPATCH line; profiles/dispatch_boundaries.txt is that output on an MI355X."""
import functools

import pytest
import torch

from oracle import hotpath as hp
from tests import bf16_emulation as em
from tests import depth_fuse_neighbours_util as fu
from tests import depth_multiview_util as mv
from tests import dispatch_boundaries as db
from tests.dispatch_boundaries import C, err, record, rnd, tok
from unimatch_amd import _abi, confidence
from unimatch_amd.ops import HipOps

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F = torch.nn.functional


@pytest.fixture(scope='module')
def ops():
    return HipOps('exact')


@pytest.fixture(scope='module')
def ops_fast():
    return HipOps('fast')


@pytest.fixture(scope='module')
def lib(ops):
    return ops.lib


@pytest.fixture(scope='module')
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


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
    """The census ids among ``names`` that counted, as a string; asserts that exactly one launch was counted among them."""
    hit = [n for n in names if counts[n]]
    assert len(hit) == 1 and counts[hit[0]] == 1, {n: counts[n] for n in names}
    return hit[0]


def scale_of(t):
    return max(1.0, t.abs().max().item())


# ================================================================== row 1: window attention, token table | arithmetic addressing
# window_attn.hip:231 -- use_tab = ntiles * 32 * 4 <= 8192: windows of more than 2048 tokens address their tokens arithmetically
# (natural order, no class-major walk, a tile range instead of a bit mask).
ATTN_GEOS = {
    # name: (h, w, win_h, win_w, shift_h, shift_w)
    'table-32x64': (32, 64, 32, 64, 0, 0),                      # exactly 2048 tokens, 64 key tiles: the last window with a table
    'arith-1x2080': (1, 2080, 1, 2080, 0, 0),                   # 65 key tiles, one row
    'arith-40x52': (40, 52, 40, 52, 0, 0),                      # 65 key tiles, 2-D
    'arith-shifted-33x64': (66, 128, 33, 64, 16, 32),           # four shifted windows of 2112 tokens, 66 key tiles: masks without the table
    'arith-shifted-1x2080': (3, 4160, 1, 2080, 0, 1040),        # shifted 1-D windows
}


def attn_inputs(name, streams):
    h, w = ATTN_GEOS[name][:2]
    return tuple(rnd(3000 + 10 * len(name) + i, streams, h * w, C, scale=1.5) for i in range(3))


def attn_case(name, streams):
    """q, k, v and the fp64 oracle's result.  Nothing is kept: the exact and the bf16 test of a case have different references."""
    h, w, wh, ww, sh, sw = ATTN_GEOS[name]
    q, k, v = attn_inputs(name, streams)
    return q, k, v, hp.window_attention(q.double(), k.double(), v.double(), h, w, wh, ww, sh, sw)


@pytest.mark.parametrize('streams', ['one', 'unsplit'])
@pytest.mark.parametrize('name', list(ATTN_GEOS))
def test_window_attention_table_and_arithmetic(ops, lib, cus, name, streams):
    """um_window_attn_fwd against hp.window_attention on one stream and on the smallest stream count whose launch um_window_attn_plan
    leaves unsplit.  (um_window_attn_fwd itself never key-splits, window_attn.hip:1353; the plan's stream count makes this launch as
    large as the layer kernel's first unsplit one.  The key-split side of the same geometry: test_merged_layer_arithmetic_key_split.)"""
    h, w, wh, ww, sh, sw = ATTN_GEOS[name]
    s = 1 if streams == 'one' else db.attn_unsplit_streams(lib, h, w, wh, ww)
    assert db.attn_uses_token_table(wh, ww) == name.startswith('table')
    assert (streams == 'one') == (db.attn_parts(lib, s, h, w, wh, ww) > 1)          # one stream of each of these would key-split
    q, k, v, want = attn_case(name, s)
    got, c = census(lib, lambda: ops.window_attention(q.to(DEV), k.to(DEV), v.to(DEV), h, w, wh, ww, sh, sw))
    variant = only(c, 'wattn_tile', 'wattn_ksplit')
    assert variant == 'wattn_tile'
    assert torch.isfinite(got).all()
    mx, gate = err(got, want)[0], 5e-5 * scale_of(want)
    record('1 attention table|arithmetic', f'{name} streams={s}', 'table' if name.startswith('table') else 'arithmetic', variant, mx, gate, cus)
    assert mx < gate, (name, s, mx)


@pytest.mark.parametrize('name', list(ATTN_GEOS))
def test_window_attention_table_and_arithmetic_fast(ops_fast, lib, cus, name):
    """The same cases on bf16 operands against the as-rounded emulation (tests/bf16_emulation.py): element bound 2 U sum p|v| / sum p
    + the exact-mode floor, mean gate from the fp32 emulation.  One stream only: um_window_attn_fwd takes the same kernel path at every
    stream count (it never key-splits), and the two emulations of the 16- and 17-stream launches would cost 6 s a case on the host."""
    h, w, wh, ww, sh, sw = ATTN_GEOS[name]
    q, k, v = attn_inputs(name, 1)
    got, c = census(lib, lambda: ops_fast.window_attention(q.to(DEV), k.to(DEV), v.to(DEV), h, w, wh, ww, sh, sw))
    variant = only(c, 'wattn_tile', 'wattn_ksplit')
    e64, bound = em.window_attention(q, k, v, h, w, wh, ww, sh, sw, torch.float64, True, want_bound=True)
    e32 = em.window_attention(q, k, v, h, w, wh, ww, sh, sw, torch.float32, True)
    floor = 5e-5 * scale_of(e64)
    st = em.gate(got, e64, e32, bound, floor, name)
    record('1 attention table|arithmetic, bf16', f'{name} streams=1', 'table' if name.startswith('table') else 'arithmetic', variant,
           st['got_max'], (bound.max().item() + floor), cus)


def test_window_attention_mask_dominance_without_the_table(ops, lib, cus):
    """A cross-class logit that beats its row by more than 100 must WIN the softmax (the reference adds -100, it does not exclude) --
    on the arithmetic path, where masked tiles are found from a tile range: the probe of
    test_window_attention_forced_rescale_and_mask_dominance in the last window of the shifted 2112-token geometry."""
    h, w, wh, ww, sh, sw = ATTN_GEOS['arith-shifted-33x64']
    assert not db.attn_uses_token_table(wh, ww)
    q, k, v = (rnd(3100 + i, 1, h * w, C) for i in range(3))
    idx, label = hp.window_index(h, w, wh, ww, sh, sw)
    win = idx.shape[0] - 1
    a = int(idx[win, 0])
    other = [int(idx[win, j]) for j in range(idx.shape[1]) if label[win, j] != label[win, 0]]
    assert other
    far = other[-1]                                 # the last key of another class: the far end of the tile range
    q[0, a] = 0.0
    q[0, a, 0] = 60.0
    k[0, :, 0] = 0.0
    k[0, far, 0] = 60.0                             # raw logit 3600 / sqrt(128) = 318 > 100 above everything else
    want = hp.window_attention(q.double(), k.double(), v.double(), h, w, wh, ww, sh, sw)
    got, c = census(lib, lambda: ops.window_attention(q.to(DEV), k.to(DEV), v.to(DEV), h, w, wh, ww, sh, sw))
    variant = only(c, 'wattn_tile', 'wattn_ksplit')
    assert variant == 'wattn_tile'
    assert (want[0, a] - v[0, far].double()).abs().max() < 1e-6                      # the masked key dominates
    assert (got[0, a].cpu().double() - v[0, far].double()).abs().max() < 1e-4
    mx, gate = err(got, want)[0], 1e-4 * scale_of(want)
    record('1 attention mask dominance', 'arith-shifted-33x64 streams=1', 'arithmetic', variant, mx, gate, cus)
    assert mx < gate


# ------------------------------------------------------------------ the merged layer (um_window_attn_qproj_merge_fwd)
class Layer:
    """Inputs, weights and the fp64 composition of one merged attention layer; ``run`` launches um_window_attn_qproj_merge_fwd."""

    def __init__(self, seed, streams, h, w, geom, rot, residual=True):
        self.s, self.h, self.w, self.geom, self.rot, self.residual = streams, h, w, geom, rot, residual
        self.m = streams * h * w
        self.x, self.xt = rnd(seed, self.m, C, scale=1.5), rnd(seed + 1, self.m, C, scale=1.5)
        self.wq, self.wk, self.wv, self.wm = (rnd(seed + 2 + i, C, C, scale=0.09) for i in range(4))
        self.norm = db.layer_norm_params(seed + 6, seed + 7)
        self.want = db.merged_layer_reference(self.x, self.xt, self.wq, self.wk, self.wv, self.wm, self.norm, streams, h, w, geom, rot,
                                              residual)

    def run(self, ops, workspace=True):
        xd, xtd = self.x.to(DEV), self.xt.to(DEV)
        wq, wk, wv, wm = (t.to(DEV) for t in (self.wq, self.wk, self.wv, self.wm))
        norm = torch.nn.LayerNorm(C).to(DEV)
        norm.load_state_dict(self.norm.state_dict())
        kv, _, n2 = ops.linear_planes(xtd, (wk, wv))
        m = self.m
        res = xd if self.residual else None
        if workspace:
            call = lambda: ops.window_attention_qproj_merge(xd, wq, (kv, m, n2, 0), (kv, m, n2, C), self.s, self.h, self.w, *self.geom,
                                                            self.rot, wm, norm, res)
        else:
            # the C ABI with a NULL workspace: the layer kernel then serves one workgroup per tile (window_attn.hip:1332).  k and v
            # are the two 128-column halves of the [NS][m][256] planes: row stride n2, plane stride m * n2 elements, v 128 elements in
            wqp, wmp = ops.weight_planes((wq,))[0], ops.weight_planes((wm,))[0]
            out = torch.empty((self.s, self.h * self.w, C), dtype=torch.float32, device=DEV)

            def call():
                rc = ops.lib.um_window_attn_qproj_merge_fwd(
                    xd.data_ptr(), wqp.data_ptr(), kv.data_ptr(), kv.data_ptr() + 2 * C, wmp.data_ptr(), norm.weight.data_ptr(),
                    norm.bias.data_ptr(), res.data_ptr() if res is not None else None, float(norm.eps), ops.WSHIFT, out.data_ptr(),
                    self.s, self.h, self.w, C, n2, m * n2, *self.geom, self.rot, ops.mode, None, 0,
                    torch.cuda.current_stream().cuda_stream)
                assert rc == 0, ops.lib.um_last_error_string()
                return out
        got, c = census(ops.lib, call)
        return got.reshape(m, C), only(c, 'wattn_tile', 'wattn_ksplit')


def check_layer(layer, ops, lib, cus, row, tag, want_parts, workspace=True):
    wh, ww = layer.geom[:2]
    parts = db.attn_parts(lib, layer.s, layer.h, layer.w, wh, ww)
    assert parts == want_parts, (tag, parts, want_parts)
    got, variant = layer.run(ops, workspace)
    assert variant == ('wattn_ksplit' if parts > 1 and workspace else 'wattn_tile'), (tag, variant, parts)
    assert torch.isfinite(got).all()
    mx, gate = err(got, layer.want)[0], 5e-5
    record(row, f'{tag} streams={layer.s} {layer.h}x{layer.w} windows {wh}x{ww} rot={layer.rot}',
           f'{parts} part(s)' + ('' if workspace else ', workspace withheld'), variant, mx, gate, cus)
    assert mx < gate, (tag, mx)


def test_merged_layer_arithmetic_key_split(ops, lib, cus):
    """The shifted 2112-token geometry through the layer kernel: key split x arithmetic addressing.  One stream: 68 query tiles in 4
    parts wherever 68 x 8 <= 2 CUs; the same call with the workspace withheld: unsplit; two streams with kv_rotate = 1: 136 tiles."""
    h, w, wh, ww, sh, sw = ATTN_GEOS['arith-shifted-33x64']
    one = Layer(3200, 1, h, w, (wh, ww, sh, sw), 0)
    check_layer(one, ops, lib, cus, '1 merged layer, arithmetic', 'arith-shifted-33x64', db.attn_split_rule(68, 66, cus))
    check_layer(one, ops, lib, cus, '1 merged layer, arithmetic', 'arith-shifted-33x64', db.attn_split_rule(68, 66, cus), workspace=False)
    two = Layer(3210, 2, h, w, (wh, ww, sh, sw), 1, residual=False)
    check_layer(two, ops, lib, cus, '1 merged layer, arithmetic', 'arith-shifted-33x64', db.attn_split_rule(136, 66, cus))
    assert db.attn_parts(lib, 1, h, w, wh, ww) > 1, 'this device key-splits neither launch: the row has lost its split side'


# ================================================================== row 2: key-split plan edges
# window_attn.hip:1100 -- while (split < 4 && total * (2 * split) <= 2 * cus && ntiles >= 4 * (2 * split)) split *= 2
@pytest.mark.parametrize('tag,h,w,wh,ww,shift,parts', [
    ('7 key tiles', 28, 16, 14, 16, (7, 0), 1),              # 224-token windows: too few tiles for two parts
    ('8 key tiles', 32, 16, 16, 16, (8, 0), 2),              # 256-token windows
    ('15 key tiles', 30, 32, 15, 32, (7, 0), 2),             # 480-token windows: too few tiles for four parts
    ('16 key tiles', 32, 32, 16, 32, (8, 0), 4),             # 512-token windows
])
def test_key_split_by_key_tiles(ops, lib, cus, tag, h, w, wh, ww, shift, parts):
    """Two shifted windows on two streams (kv_rotate = 1): 8 or 16 query tiles, few enough for any device of 32 CUs or more to split as
    far as the key tiles allow."""
    assert cus >= 32
    layer = Layer(3300 + wh, 2, h, w, (wh, ww) + shift, 1)
    check_layer(layer, ops, lib, cus, '2 key split by key tiles', tag, parts)


def test_key_split_by_tile_count(ops, lib, cus):
    """window_attn.hip:1100, 1125 -- stacked 512-token windows (4 query tiles each): the last count of windows that splits in four,
    the first that splits in two, the last that splits in two, the first that does not.  With 256 CUs: 32 | 33 and 64 | 65 windows =
    128 | 132 and 256 | 260 tiles (a launch's tile count moves in steps of its windows' query tiles: see STEP_WINDOW)."""
    steps = db.attn_split_steps(lib)
    assert [s[2:] for s in steps] == [(4, 2), (2, 1)], steps
    wh, ww = db.STEP_WINDOW
    for below, above, p_below, p_above in steps:
        assert 4 * below * p_below <= 2 * cus < 4 * above * p_below        # p_below parts were granted at split = p_below / 2
        for k, parts in ((below, p_below), (above, p_above)):
            layer = Layer(3400 + k, 1, wh * k, ww, (wh, ww, wh // 2, 0), 0)
            check_layer(layer, ops, lib, cus, '2 key split by tile count', f'{4 * k} tiles', parts)


# ================================================================== row 3: FFN hidden split
# ffn.hip:983 -- while (split < 4 && tiles * (2 * split) <= cus && nslice % (2 * split) == 0 && nslice / (2 * split) >= 4) split *= 2
class Ffn:
    def __init__(self, m, hidden):
        self.m, self.hidden = m, hidden
        self.x, self.y = rnd(80, m, 128, scale=1.5), rnd(81, m, 128, scale=1.5)
        self.w1, self.w2 = rnd(82, hidden, 256, scale=0.08), rnd(83, 128, hidden, scale=0.06)
        self.norm = db.layer_norm_params(84, 85)
        self.want = db.ffn_reference(self.x, self.y, self.w1, self.w2, self.norm)

    def device(self):
        norm = torch.nn.LayerNorm(128).to(DEV)
        norm.load_state_dict(self.norm.state_dict())
        return self.x.to(DEV), self.y.to(DEV), self.w1.to(DEV), self.w2.to(DEV), norm


KV_WEIGHTS = tuple(rnd(1410 + i, 128, 128, scale=0.09) for i in range(4))


def check_kv(row, case, got, kv, side, variant, cus):
    """``out`` and the four k | v projections of it (hi + lo planes recombined) against fp64: the gates of test_fused_ffn_kernel (max) and of
    test_ffn_with_the_next_blocks_kv_projection (means)."""
    m = case.m
    e = err(got, case.want)
    planes = kv.view(torch.float16).view(2, 4, m, 128).double().sum(0).cpu()
    ekv = max(err(planes[j], case.want @ KV_WEIGHTS[j].double().t())[1] for j in range(4))
    record(row, f'm={m} hidden={case.hidden}, out', side, variant, e[0], 3e-5, cus)
    record(row, f'm={m} hidden={case.hidden}, k|v planes (mean)', side, variant, ekv, 4e-6, cus)
    assert torch.isfinite(got).all() and e[0] < 3e-5 and e[1] < 2e-6 and ekv < 4e-6, (m, case.hidden, side, e, ekv)


def check_ffn(ops, lib, cus, row, m, hidden, want_split):
    """um_ffn_ws_fwd and um_ffn_kv_fwd (both given the workspace um_ffn_split_workspace_bytes asks for) at one geometry: the split the
    size function reports is the one meant, the census names the kernel -- ffn_hsplit where the launch splits (um_ffn_kv_fwd then runs
    um_kv4_fwd as a second launch, ffn.hip:1091), ffn_tile where it does not (with the k | v epilogue fused, ffn.hip:1076)."""
    split = db.ffn_split(lib, m, hidden)
    assert split == want_split == db.ffn_split_rule(m, hidden, cus), (m, hidden, split, want_split)
    expect = 'ffn_hsplit' if split > 1 else 'ffn_tile'
    case = Ffn(m, hidden)
    got, c = census(lib, lambda: ops.ffn_ln(*case.device()))
    variant = only(c, 'ffn_tile', 'ffn_hsplit')
    assert variant == expect, (m, hidden, variant)
    assert torch.isfinite(got).all()
    mx = err(got, case.want)[0]
    record(row, f'm={m} hidden={hidden}', f'split {split}', variant, mx, 3e-5, cus)
    assert mx < 3e-5, (m, hidden, mx)
    wsd = tuple(t.to(DEV) for t in KV_WEIGHTS)
    (got, kv), c = census(lib, lambda: ops.ffn_ln_kv(*case.device(), wsd))
    variant = only(c, 'ffn_tile', 'ffn_hsplit')
    assert variant == expect, (m, hidden, variant, 'um_ffn_kv_fwd')
    check_kv(row + ', um_ffn_kv_fwd', case, got, kv, f'split {split}', variant + (' + kv4' if split > 1 else ' with the k|v epilogue'), cus)


def test_ffn_split_by_token_count(ops, lib, cus):
    """um_ffn_ws_fwd and um_ffn_kv_fwd at hidden 1024 on both sides of every step um_ffn_split_workspace_bytes reports for this device
    (256 CUs: m = 8192 | 8193 splits 4 | 2, m = 16384 | 16385 splits 2 | not at all -- there um_ffn_kv_fwd changes from the split FFN
    plus um_kv4_fwd to the fused kernel, whose last tile then holds one row), against the fp64 reference of test_fused_ffn_kernel."""
    steps = db.ffn_split_steps(lib, 1024)
    assert [s[2:] for s in steps] == [(4, 2), (2, 1)], steps
    for below, above, s_below, s_above in steps:
        check_ffn(ops, lib, cus, '3 FFN split by token count', below, 1024, s_below)
        check_ffn(ops, lib, cus, '3 FFN split by token count', above, 1024, s_above)


@pytest.mark.parametrize('hidden,split', [(64, 1), (96, 1), (128, 1), (256, 2), (320, 2), (512, 4)])
def test_ffn_split_by_slice_count(ops, lib, cus, hidden, split):
    """One 128-token tile: 2, 3, 4 slices of the hidden width do not split; 8 split in two (four would leave 2 per part); 10 split in
    two (5 per part: an odd remainder); 16 split in four.  um_ffn_ws_fwd and um_ffn_kv_fwd."""
    assert cus >= 4
    check_ffn(ops, lib, cus, '3 FFN split by slice count', 128, hidden, split)


@pytest.mark.parametrize('hidden', [1024, 320])
def test_ffn_kv_without_workspace_takes_the_fused_kernel(ops, lib, cus, hidden):
    """um_ffn_kv_fwd at a geometry whose FFN would split (m = 128), called through the C ABI with a NULL workspace: no split is possible
    (ffn.hip:1066), so the call takes the unsplit kernel with the fused k | v epilogue (ffn.hip:971, 1076).  Against fp64."""
    m = 128
    split = db.ffn_split(lib, m, hidden)
    assert split > 1, 'this device does not split one tile: the row has lost its split side'
    case = Ffn(m, hidden)
    x, y, w1, w2, norm = case.device()
    wsd = tuple(t.to(DEV) for t in KV_WEIGHTS)
    w1p, w2p, wc = ops.weight_planes((w1,))[0], ops.weight_planes((w2,))[0], ops.kv4_weight_planes(wsd)
    out = torch.empty((m, 128), dtype=torch.float32, device=DEV)
    kv = torch.empty(lib.um_planes_bytes(4 * m, 128, ops.mode), dtype=torch.uint8, device=DEV)
    rc, c = census(lib, lambda: lib.um_ffn_kv_fwd(
        x.data_ptr(), y.data_ptr(), w1p.data_ptr(), w2p.data_ptr(), m, hidden, ops.WSHIFT, norm.weight.data_ptr(), norm.bias.data_ptr(),
        float(norm.eps), out.data_ptr(), wc.data_ptr(), kv.data_ptr(), ops.mode, None, 0, torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.um_last_error_string()
    variant = only(c, 'ffn_tile', 'ffn_hsplit')
    assert variant == 'ffn_tile'
    check_kv('3 FFN k|v epilogue, NULL workspace', case, out, kv, f'split {split} withheld', variant + ' with the k|v epilogue', cus)


# ================================================================== row 4: the per-pixel local kernels past their grid cap
# local_pixel.h:105 -- pixel_grid_blocks caps the grid at 4096 workgroups of 4 waves; past 16384 pixels a wave takes a second trip of
# pid += gridDim.x * 4 (local_ops.hip: local_corr_softmax_kernel :38, prop_local_attn_kernel :294, depth_corr_softmax{,_box}{,_stats}_kernel
# :477, :539, local_corr_with_flow_dilated_kernel :733).  The multi-view sweeps past the same cap: row 8.
CAP_SIZES = [(128, 128), (129, 128)]              # 16384 pixels: the last one-trip map | 16512: 32 workgroups go round again


def _side(h, w):
    trips = db.pixel_grid_trips(h * w)
    assert trips == (1 if h * w <= 16384 else 2)
    return f'{trips} trip(s)'


@pytest.mark.parametrize('hw', CAP_SIZES)
@pytest.mark.parametrize('one_d,radius', [(False, 2), (True, 4)])
def test_grid_cap_local_corr_softmax(ops, lib, cus, hw, one_d, radius):
    """um_local_corr_softmax on local_corr_softmax_kernel (radius 2: the matrix-core kernel serves radius 4 only)."""
    h, w = hw
    f0, f1 = db.local_features(1, h, w)
    want = hp.local_corr_softmax(f0.double(), f1.double(), radius, one_d)
    got, c = census(lib, lambda: ops.local_corr_softmax(tok(f0).to(DEV), tok(f1).to(DEV), h, w, radius, one_d=one_d))
    variant = only(c, 'k3_valu', 'k3_mfma')
    assert variant == 'k3_valu'
    mx = err(got, want)[0]
    record('4 grid cap, local softmax', f'1x{h}x{w} radius {radius} {"1-D" if one_d else "2-D"}', _side(h, w), variant, mx, 2e-4, cus)
    assert mx < 2e-4


@pytest.mark.parametrize('hw', CAP_SIZES)
@pytest.mark.parametrize('vch', [1, 2])
def test_grid_cap_prop_local(ops, cus, hw, vch):
    """um_prop_local_attn (no census id: the entry point has one kernel)."""
    h, w = hw
    q, k = db.local_features(1, h, w)
    val = rnd(3500 + vch, 1, vch, h, w, scale=3.0)
    want = db.prop_local_reference(q.double(), k.double(), val.double(), 2)
    got = ops.prop_local(tok(q).to(DEV), tok(k).to(DEV), val.to(DEV), h, w, 2)
    mx = err(got, want)[0]
    record('4 grid cap, prop_local', f'1x{h}x{w} radius 2, {vch} value channel(s)', _side(h, w), 'prop_local_attn_kernel', mx, 2e-4, cus)
    assert mx < 2e-4


def sweep_stats_reference(b, h, w, nd):
    """float64 host restatement of the sweep's statistics (peak_radius 1) -> (statistics, prob [B, D, h, w], clear [B, h, w]): ``clear``
    marks the pixels none of whose candidates lands within 1e-3 of a coordinate at which ``in_view`` changes (x = -1 or w, y = -1 or h),
    the rule of tests/test_depth_stats_gpu.py."""
    f0, f1 = db.sweep_features(b, h, w)
    _, _, cam = db.sweep_camera(b, h, w)
    cam, cand = cam.double(), db.sweep_candidates(nd).double()
    logits, seen = confidence.depth_match_logits_host(tok(f0).double(), tok(f1).double(), h, w, cam, cand)
    prob = torch.softmax(logits, 1)
    sx, sy = confidence.depth_sample_coords_host(h, w, cam, cand)
    near = torch.zeros_like(sx, dtype=torch.bool)
    for coord, hi in ((sx, w), (sy, h)):
        for edge in (-1.0, float(hi)):
            near |= (coord - edge).abs() < 1e-3
    return confidence.depth_stats_from_prob_host(prob, cand, seen, 1), prob, ~near.any(1)


def sweep_device(ops, b, h, w, nd, argmax=False, stats=False):
    f0, f1 = db.sweep_features(b, h, w)
    _, _, cam = db.sweep_camera(b, h, w)
    return ops.depth_corr_softmax(tok(f0).to(DEV), tok(f1).to(DEV), h, w, cam.to(DEV), db.sweep_candidates(nd).to(DEV), from_argmax=argmax,
                                  stats=stats)


@pytest.mark.parametrize('hw', CAP_SIZES)
@pytest.mark.parametrize('nd', [16, 65])
def test_grid_cap_plane_sweep(ops, cus, hw, nd):
    """um_depth_corr_softmax and um_depth_corr_softmax_stats on the box kernel (16 candidates) and the gather kernel (65; the rule is
    local_ops.hip:812, 841: ``num_candidates <= 64``).  The statistics against the float64 host restatement under the gates of
    tests/test_depth_stats_gpu.py: 2e-4 x the scale of each plane."""
    h, w = hw
    kernel = 'box' if db.depth_uses_box_kernel(nd) else 'gather'
    want = db.sweep_reference(1, h, w, nd, False)
    gate = 2e-4 * scale_of(want)
    got = sweep_device(ops, 1, h, w, nd)
    mx = err(got, want)[0]
    record('4 grid cap, plane sweep', f'1x{h}x{w} {nd} candidates', _side(h, w), f'depth_corr_softmax {kernel}', mx, gate, cus)
    assert mx < gate
    out, planes, index = sweep_device(ops, 1, h, w, nd, stats=True)
    mx = err(out, want)[0]
    record('4 grid cap, plane sweep + stats', f'1x{h}x{w} {nd} candidates, out', _side(h, w), f'depth_corr_softmax_stats {kernel}', mx, gate, cus)
    assert mx < gate
    ref, prob, clear = sweep_stats_reference(1, h, w, nd)
    cand = db.sweep_candidates(nd)
    scales = {'max_prob': 1.0, 'entropy': max(1.0, torch.log(torch.tensor(float(nd))).item()),
              'variance': (cand.max() - cand.min()).item() ** 2, 'peak_mass': 1.0}
    for i, name in enumerate(('max_prob', 'entropy', 'variance', 'peak_mass')):
        mx = err(planes[:, i], getattr(ref, name))[0]
        record('4 grid cap, plane sweep + stats', f'1x{h}x{w} {nd} candidates, {name}', _side(h, w), f'depth_corr_softmax_stats {kernel}', mx,
               2e-4 * scales[name], cus)
        assert mx <= 2e-4 * scales[name], (name, mx)
    # the int32 planes under the rules of tests/test_depth_stats_gpu.py: best in range and, by VALUE, a maximum of the float64 row (no
    # row excluded); in_view equal to the float64 count wherever no candidate sits on a coordinate at which the count changes
    best, seen = index[:, 0].long().cpu(), index[:, 1].cpu()
    assert bool((best >= 0).all()) and bool((best < nd).all())
    short = (prob.amax(1) - prob.gather(1, best[:, None])[:, 0]).max().item()
    record('4 grid cap, plane sweep + stats', f'1x{h}x{w} {nd} candidates, best (probability short of the row maximum)', _side(h, w),
           f'depth_corr_softmax_stats {kernel}', short, 2e-4, cus)
    assert short <= 2e-4
    kept = clear.float().mean().item()
    assert kept >= 0.95, kept
    wrong = (seen[clear] != ref.in_view[clear]).float().mean().item()
    record('4 grid cap, plane sweep + stats', f'1x{h}x{w} {nd} candidates, in_view (mismatches among the {kept:.3f} of the pixels compared)', _side(h, w),
           f'depth_corr_softmax_stats {kernel}', wrong, 0.0, cus)
    assert torch.equal(seen[clear], ref.in_view[clear])
    assert bool((seen >= 0).all()) and bool((seen <= nd).all())


@pytest.mark.parametrize('hw', CAP_SIZES)
def test_grid_cap_dilated_cost_volume(ops, lib, cus, hw):
    """um_local_corr_with_flow_dilated at dilation 2 (fractional, exactly integer and far out-of-image flow)."""
    h, w = hw
    f0, f1 = db.local_features(1, h, w)
    flow = rnd(3600, 1, 2, h, w, scale=2.5)
    flow[:, :, 0, 0] = 3.0
    flow[:, :, -1, -1] = 1000.0
    want = hp.local_corr_with_flow_dilated(f0.double(), f1.double(), flow.double(), 2, 2)
    got, c = census(lib, lambda: ops.local_corr_with_flow(tok(f0).to(DEV), tok(f1).to(DEV), flow.to(DEV), h, w, 2, dilation=2))
    variant = only(c, 'k4_valu', 'k4_mfma')
    assert variant == 'k4_valu'
    mx, gate = err(got, want)[0], 1e-4 * scale_of(want)
    record('4 grid cap, dilated cost volume', f'1x{h}x{w} radius 2 dilation 2', _side(h, w), variant, mx, gate, cus)
    assert mx < gate


def test_grid_cap_cost_volume_at_dilation_one(ops, lib, cus):
    """um_local_corr_with_flow walks 16 pixels per wave, so its cap (local_ops.hip:695-698) sits at 4096 x 4 x 16 = 262144 pixels:
    2 x 363 x 362 = 262812 pixels send 42 waves round again, and the second sample starts in mid-block.  134 MB per feature map; the
    fp64 oracle takes 3 s.  Radius 1: the matrix-core kernel serves radius 4 only.  (The one-trip side is every other cost-volume test.)"""
    b, h, w = 2, 363, 362
    assert db.pixel_grid_trips((b * h * w + 15) // 16) == 2 and db.pixel_grid_trips((b * 362 * 362 + 15) // 16) == 1
    f0, f1 = db.make_local_features(b, h, w)                     # 134 MB each: built here, not kept
    flow = rnd(3650, b, 2, h, w, scale=2.5)
    flow[:, :, 0, 0] = 3.0
    flow[:, :, -1, -1] = 1000.0
    want = hp.local_corr_with_flow(f0.double(), f1.double(), flow.double(), 1)
    got, c = census(lib, lambda: ops.local_corr_with_flow(tok(f0).to(DEV), tok(f1).to(DEV), flow.to(DEV), h, w, 1))
    variant = only(c, 'k4_valu', 'k4_mfma')
    assert variant == 'k4_valu'
    mx, gate = err(got, want)[0], 1e-4 * scale_of(want)
    record('4 grid cap, cost volume', f'{b}x{h}x{w} radius 1', '2 trip(s)', variant, mx, gate, cus)
    assert mx < gate


# ================================================================== row 5: the upper half of the tap and candidate range
# LOCAL_MAX_ROUNDS 8 (local_pixel.h:7): up to 128 taps or candidates, refused beyond (local_ops.hip:673, :792, :806, :831).
@pytest.mark.parametrize('b,h,w', [(2, 13, 19), (1, 3, 4)])                 # 494 pixels | a map smaller than every window below
def test_tap_range_local_corr_softmax(ops, lib, cus, b, h, w):
    """2-D radius 5 (121 taps: 8 rounds, 7 idle slots) and 1-D radius 41 and 63 (83 and 127 taps)."""
    f0, f1 = db.local_features(b, h, w)
    t0, t1 = tok(f0).to(DEV), tok(f1).to(DEV)
    for one_d, radius in ((False, 5), (True, 41), (True, 63)):
        taps = 2 * radius + 1 if one_d else (2 * radius + 1) ** 2
        assert taps <= db.LOCAL_MAX_TAPS
        want = hp.local_corr_softmax(f0.double(), f1.double(), radius, one_d)
        got, c = census(lib, lambda: ops.local_corr_softmax(t0, t1, h, w, radius, one_d=one_d))
        variant = only(c, 'k3_valu', 'k3_mfma')
        mx = err(got, want)[0]
        record('5 tap range, local softmax', f'{b}x{h}x{w} radius {radius} {"1-D" if one_d else "2-D"}', f'{taps} taps of 128', variant, mx,
               2e-4, cus)
        assert variant == 'k3_valu' and mx < 2e-4, (radius, one_d, mx)


@pytest.mark.parametrize('b,h,w', [(2, 13, 19), (1, 3, 4)])
@pytest.mark.parametrize('vch', [1, 2])
def test_tap_range_prop_local(ops, cus, b, h, w, vch):
    q, k = db.local_features(b, h, w)
    val = rnd(3700 + vch, b, vch, h, w, scale=3.0)
    want = db.prop_local_reference(q.double(), k.double(), val.double(), 5)
    got = ops.prop_local(tok(q).to(DEV), tok(k).to(DEV), val.to(DEV), h, w, 5)
    mx = err(got, want)[0]
    record('5 tap range, prop_local', f'{b}x{h}x{w} radius 5, {vch} value channel(s)', '121 taps of 128', 'prop_local_attn_kernel', mx, 2e-4,
           cus)
    assert mx < 2e-4


@pytest.mark.parametrize('argmax', [False, True])
@pytest.mark.parametrize('nd', db.SWEEP_COUNTS)
def test_candidate_range_plane_sweep(ops, cus, nd, argmax):
    """1, 16, 17 candidates (the edges of a 16-slot round), 64 | 65 (box | gather kernel), 128 (the limit); soft read-out and arg-max.
    The arg-max rule is the existing one -- at most 1 % of the pixels differ by more than 1e-6 -- and
    tests/test_dispatch_boundaries_cpu.py shows the fp32 oracle inside it on these inputs."""
    b, h, w = db.SWEEP_SMALL
    kernel = 'box' if db.depth_uses_box_kernel(nd) else 'gather'
    want = db.sweep_reference(b, h, w, nd, argmax)
    got = sweep_device(ops, b, h, w, nd, argmax=argmax)
    assert torch.isfinite(got).all()
    if argmax:
        off = (got.cpu().double() - want).abs().gt(1e-6).float().mean().item()
        record('5 candidate range, arg-max', f'{b}x{h}x{w} {nd} candidates', f'{nd} of 128', f'depth_corr_softmax {kernel}', off, 0.01, cus)
        assert off < 0.01, (nd, off)
    else:
        mx, gate = err(got, want)[0], 2e-4 * scale_of(want)
        record('5 candidate range', f'{b}x{h}x{w} {nd} candidates', f'{nd} of 128', f'depth_corr_softmax {kernel}', mx, gate, cus)
        assert mx < gate, (nd, mx)


def test_refusals_one_step_beyond_the_range(ops, lib, cus):
    """Radius 6 (169 taps), 1-D radius 64 (129 taps), 129 candidates, and the cost volume's radius 5: UM_ERR_UNSUPPORTED with a message,
    no launch counted, the outputs untouched."""
    b, h, w = 1, 8, 8
    f0, f1 = (tok(t).to(DEV) for t in db.local_features(b, h, w))
    _, _, cam = db.sweep_camera(b, h, w)
    cam, cand = cam.to(DEV), db.sweep_candidates(129).to(DEV)
    val, flow = rnd(1, b, 2, h, w).to(DEV), rnd(2, b, 2, h, w).to(DEV)
    out = torch.full((b, 121, h, w), float('nan'), device=DEV)
    stats, index = torch.empty(b, 4, h, w, device=DEV), torch.empty(b, 2, h, w, dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    calls = {
        '2-D radius 6': lambda: lib.um_local_corr_softmax(p(f0), p(f1), p(out), b, h, w, C, 6, 0, st),
        '1-D radius 64': lambda: lib.um_local_corr_softmax(p(f0), p(f1), p(out), b, h, w, C, 64, 1, st),
        'prop_local radius 6': lambda: lib.um_prop_local_attn(p(f0), p(f1), p(val), p(out), b, h, w, C, 2, 6, st),
        '129 candidates': lambda: lib.um_depth_corr_softmax(p(f0), p(f1), p(cam), p(cand), p(out), b, h, w, C, 129, 0, st),
        '129 candidates, stats': lambda: lib.um_depth_corr_softmax_stats(p(f0), p(f1), p(cam), p(cand), p(out), p(stats), p(index), b, h, w, C,
                                                                        129, 0, 1, st),
        'cost volume radius 5': lambda: lib.um_local_corr_with_flow(p(f0), p(f1), p(flow), p(out), b, h, w, C, 5, st),
        'dilated cost volume radius 5': lambda: lib.um_local_corr_with_flow_dilated(p(f0), p(f1), p(flow), p(out), b, h, w, C, 5, 2, st),
    }
    for what, call in calls.items():
        rc, c = census(lib, call)
        assert rc == db.UM_ERR_UNSUPPORTED and lib.um_last_error_string(), (what, rc)
        assert all(v == 0 for v in c.values()), (what, c)
        record('5 refusals', what, 'one step beyond', f'refused ({rc})', 0.0, 0.0, cus)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ================================================================== row 6: conv_pick
# conv.hip:1189-1209.  Every case: um_conv2d_fwd with its epilogue statistics against fp64 conv2d; the census names the kernel; the
# part count um_conv_stats_parts reports is the closed form of THAT kernel; the statistics feed um_nhwc_instance_norm (where the norm
# serves the channel count), which proves that the part count agrees with the launch.
CONV_CASES = [
    # tag, (b, cin, cout, h, w, kh, kw, stride, ph, pw), kind
    ('255 output pixels', (2, 64, 64, 15, 17, 3, 3, 1, 1, 1), 'generic'),          # :1199 ho * wo >= 256
    ('256 output pixels', (2, 64, 64, 16, 16, 3, 3, 1, 1, 1), 'rows'),
    ('tiles 37 % image', (2, 64, 64, 17, 33, 3, 3, 1, 1, 1), 'rows'),              # :1203 4 ho wo >= 3 tiled
    ('tiles all image', (2, 64, 64, 24, 32, 3, 3, 1, 1, 1), 'patch'),
    ('tiles 5/8 image, rows ragged', (2, 64, 64, 5, 64, 3, 3, 1, 1, 1), 'rows'),
    ('tiles 6/8 image, rows ragged', (2, 64, 64, 6, 64, 3, 3, 1, 1, 1), 'patch'),
    ('tiles 47/64 image, columns ragged', (2, 64, 64, 8, 47, 3, 3, 1, 1, 1), 'rows'),
    ('tiles 48/64 image, columns ragged', (2, 64, 64, 8, 48, 3, 3, 1, 1, 1), 'patch'),
    ('1x5, 128 outputs', (1, 64, 128, 16, 16, 1, 5, 1, 0, 2), 'rows'),             # :1200 five-tap rows need NT = 4
    ('1x5, 96 outputs', (1, 64, 96, 16, 16, 1, 5, 1, 0, 2), 'generic'),
    ('5x1, 128 outputs', (1, 64, 128, 16, 16, 5, 1, 1, 2, 0), 'generic'),
    ('5x1, 96 outputs', (1, 64, 96, 16, 16, 5, 1, 1, 2, 0), 'generic'),
] + [
    # :1191 the tile width follows cout (2 | 2 | 2 | 2 | 3 | 4 | 4 | 3 | 4 | 4), :1205 up to 32 outputs drop the patch kernel to NT = 1
    (f'cout {cout} on a {kind} map', (1, 64, cout, h, w, 3, 3, 1, 1, 1), kind)
    for kind, (h, w) in (('patch', (16, 32)), ('generic', (9, 11))) for cout in (4, 32, 36, 64, 96, 128, 160, 192, 200, 256)
]
CONV_CENSUS = {'patch': 'conv_patch', 'rows': 'conv_rows', 'generic': 'conv_generic'}


@pytest.mark.parametrize('tag,geo,kind', CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_pick(ops, lib, cus, tag, geo, kind):
    """The census observes the kernel FAMILY.  No id exists for the tile width: the NT of a record line is what conv.hip:1191 gives for
    the row's ``cout`` (the row is placed by it), not an observation -- except NT = 1 against NT >= 2 on the patch kernel, which
    um_conv2d_norm_supported tells apart."""
    b, cin, cout, h, w, kh, kw, stride, ph, pw = geo
    want_kind, nt = db.conv_kind(h, w, cout, kh, kw, stride, ph, pw)
    assert want_kind == kind, (tag, want_kind)
    x = rnd(3800, b, cin, h, w, scale=1.5)
    wt = rnd(3801, cout, cin, kh, kw, scale=(2.0 / (cin * kh * kw)) ** 0.5)
    bs = 3.0 * rnd(3802, cout)                                       # a large mean per channel, for the statistics
    want = F.conv2d(x.double(), wt.double(), bs.double(), stride=stride, padding=(ph, pw))
    planes, _ = ops.nchw_to_nhwc(x.to(DEV).contiguous(), want_planes=True, want_f32=False)
    (got, ho, wo), c = census(lib, lambda: ops.conv2d_nhwc((planes, b, h, w, cin), wt.to(DEV), bs.to(DEV), stride, (ph, pw), stats=True))
    variant = only(c, 'conv_patch', 'conv_rows', 'conv_generic')
    assert variant == CONV_CENSUS[kind] and c['conv_patch_norm'] == 0, (tag, variant)
    assert (ho, wo) == tuple(want.shape[-2:])
    st, parts = ops.last_conv_stats
    assert parts == lib.um_conv_stats_parts(h, w, cout, kh, kw, stride, ph, pw) == db.conv_parts(kind, ho, wo), (tag, parts)
    # the on-load kernel is offered for the patch kernel's 64-column tiles and wider -- NT = 1 (cout <= 32) is told from NT = 2 by it
    assert lib.um_conv2d_norm_supported(h, w, cin, cout, kh, kw, stride, ph, pw, 0) == int(kind == 'patch' and nt >= 2), (tag, nt)
    mx, gate = err(got.view(b, ho, wo, cout).permute(0, 3, 1, 2), want)[0], 3e-6 * scale_of(want)
    record('6 conv_pick', f'{tag}: {b}x{cin}x{h}x{w} -> {cout}, {kh}x{kw}', f'{kind}, NT={nt} by the rule', variant, mx, gate, cus)
    assert mx < gate, (tag, mx)
    if cout % 8 == 0:                                                # um_nhwc_instance_norm: channels a multiple of 8
        _, normed = ops.nhwc_norm(got, b, ho * wo, relu=False, want_planes=False, want_f32=True, conv_stats=(st, parts))
        _, own = ops.nhwc_norm(got, b, ho * wo, relu=False, want_planes=False, want_f32=True)
        e = err(normed.view(b, ho, wo, cout).permute(0, 3, 1, 2), F.instance_norm(want))[0]
        record('6 conv_pick, statistics -> norm', f'{tag}: {parts} parts per image', f'{kind}, NT={nt} by the rule', variant, e, 3e-5, cus)
        assert e < 3e-5 and err(normed, own)[0] < 1e-5, (tag, e)


@pytest.mark.parametrize('tag,geo,kind', [c for c in CONV_CASES if c[1][5] != c[1][6]], ids=[c[0] for c in CONV_CASES if c[1][5] != c[1][6]])
def test_conv_pick_through_conv_ex(ops, lib, cus, tag, geo, kind):
    """The GRU's separable gates reach conv_pick through um_conv2d_ex (strided operand planes, a fused activation)."""
    b, cin, cout, h, w, kh, kw, stride, ph, pw = geo
    x = rnd(3810, b, cin, h, w, scale=1.2)
    wt = rnd(3811, cout, cin, kh, kw, scale=(2.0 / (cin * kh * kw)) ** 0.5)
    bs = rnd(3812, cout)
    pre = F.conv2d(x.double(), wt.double(), bs.double(), stride=stride, padding=(ph, pw))
    want = torch.tanh(pre)
    rows = b * h * w
    src = ops.planes_buffer(rows, cin)
    ops.nhwc_gate(0, x.permute(0, 2, 3, 1).reshape(rows, cin).contiguous().to(DEV), src, cin, 0, rows, cin)
    out = torch.empty((rows, cout), dtype=torch.float32, device=DEV)
    wb = (ops.conv_weight_planes_from(wt.to(DEV)), bs.to(DEV))
    _, c = census(lib, lambda: ops.conv_ex((src, cin, 0, cin), (b, h, w), wb, (kh, kw), stride, (ph, pw), 3, out=(out, cout, 0)))
    variant = only(c, 'conv_patch', 'conv_rows', 'conv_generic')
    assert variant == CONV_CENSUS[kind], (tag, variant)
    mx, gate = err(out.view(b, h, w, cout).permute(0, 3, 1, 2), want)[0], 3e-6 * scale_of(pre)
    record('6 conv_pick, um_conv2d_ex', f'{tag}: {b}x{cin}x{h}x{w} -> {cout}, {kh}x{kw}, tanh', kind, variant, mx, gate, cus)
    assert mx < gate, (tag, mx)


def test_conv_refuses_two_output_channels(ops, lib, cus):
    """``cout % 4 != 0`` is a bad argument (conv.hip:1268): the flow head's two outputs are served padded to four, the narrowest case of
    the table above."""
    x = rnd(3820, 1, 32, 8, 8)
    planes, _ = ops.nchw_to_nhwc(x.to(DEV).contiguous(), want_planes=True, want_f32=False)
    with pytest.raises(ValueError, match='code -1'):
        ops.conv2d_nhwc((planes, 1, 8, 8, 32), rnd(3821, 2, 32, 3, 3).to(DEV))


@pytest.mark.parametrize('hw,supported', [((6, 64), 1), ((5, 64), 0), ((8, 48), 1), ((8, 47), 0)])
def test_norm_on_load_follows_the_patch_rule(ops, lib, cus, hw, supported):
    """um_conv2d_norm_supported on both sides of the 3/4 tile-area rule; on the supported side HipOps.conv2d_nhwc_normed
    (um_nhwc_stats_finalize + um_conv2d_norm_fwd on the statistics the first convolution left) against fp64
    conv2d(relu(instance_norm(conv2d(x)))) under the gate of test_on_load_convolution_matches_fp64.  (The refused side's return code:
    tests/test_conv_norm_on_load_gpu.py.)"""
    c, b = 64, 2
    h, w = hw
    w1, w2 = rnd(97, c, c, 3, 3, scale=0.06), rnd(197, c, c, 3, 3, scale=0.06)
    assert lib.um_conv2d_norm_supported(h, w, c, c, 3, 3, 1, 1, 1, 0) == supported == int(ops.conv2d_norm_supported(h, w, c, w2))
    if not supported:
        record('6 norm on load', f'{b}x{c}x{h}x{w}', 'below 3/4 of the tiles', 'not offered', 0.0, 0.0, cus)
        return
    x, bs = rnd(96, b, c, h, w, scale=1.5), 3.0 * rnd(98, c)         # a bias of several units: a halo pixel must be 0, not norm(0)
    planes, _ = ops.nchw_to_nhwc(x.to(DEV).contiguous(), want_planes=True, want_f32=False)
    t, _, _ = ops.conv2d_nhwc((planes, b, h, w, c), w1.to(DEV), bs.to(DEV), 1, (1, 1), stats=True)
    (got, _, _), cen = census(lib, lambda: ops.conv2d_nhwc_normed(t, ops.last_conv_stats, (b, h, w, c), w2.to(DEV)))
    assert cen['conv_patch_norm'] == 1 and only(cen, 'conv_patch', 'conv_rows', 'conv_generic') == 'conv_patch', cen
    want = F.conv2d(F.instance_norm(F.conv2d(x.double(), w1.double(), bs.double(), padding=1)).relu(), w2.double(), None, padding=1)
    mx, gate = err(got.view(b, h, w, c).permute(0, 3, 1, 2), want)[0], 4e-6 * scale_of(want)
    record('6 norm on load', f'{b}x{c}x{h}x{w}', 'at 3/4 of the tiles', 'conv_patch_norm', mx, gate, cus)
    assert mx < gate


@pytest.mark.parametrize('cin,cout,supported', [(128, 128, 1), (160, 128, 0), (96, 192, 1), (64, 64, 0)])
def test_entry_kernel_follows_its_conditions(ops, lib, cus, cin, cout, supported):
    """um_conv2d_entry_supported on both sides of its own conditions (conv.hip:1232-1241: at most 128 input channels; 96- and 128-wide
    tiles); on the supported side HipOps.conv2d_entry (um_conv2d_entry_fwd: the block input relu(norm(u) + S) is never written) against
    fp64 under the gate of test_entry_convolution_matches_fp64."""
    (h, w), b = (17, 33), 2
    w1, wpj = rnd(197, cout, cin, 3, 3, scale=0.06), rnd(297, cout, cin, 1, 1, scale=0.15)
    assert lib.um_conv2d_entry_supported(h, w, cin, cout, 3, 3, 2, 1, 1, 0) == supported == int(ops.conv2d_entry_supported(h, w, cin, w1, wpj))
    if not supported:
        record('6 entry kernel', f'{b}x{cin}x{h}x{w} -> {cout}', 'outside', 'not offered', 0.0, 0.0, cus)
        return
    s = rnd(96, b, cin, h, w, scale=1.5)                             # S: the identity shortcut, and the producing convolution's input
    w0, b0, bpj = rnd(97, cin, cin, 3, 3, scale=0.06), 3.0 * rnd(98, cin), 2.0 * rnd(99, cout)
    sp, _ = ops.nchw_to_nhwc(s.to(DEV).contiguous(), want_planes=True, want_f32=False)
    u, _, _ = ops.conv2d_nhwc((sp, b, h, w, cin), w0.to(DEV), b0.to(DEV), 1, (1, 1), stats=True)
    (t, d, ho, wo, _, _), cen = census(lib, lambda: ops.conv2d_entry(u, ops.last_conv_stats, sp, (b, h, w, cin), w1.to(DEV), wpj.to(DEV),
                                                                   bpj.to(DEV)))
    assert only(cen, 'conv_patch', 'conv_rows', 'conv_generic') == 'conv_generic' and cen['conv_patch_norm'] == 0, cen
    x = (F.instance_norm(F.conv2d(s.double(), w0.double(), b0.double(), padding=1)).relu() + s.double()).relu()
    assert (ho, wo) == ((h - 1) // 2 + 1, (w - 1) // 2 + 1)
    for name, got, want in (('t', t, F.conv2d(x, w1.double(), None, stride=2, padding=1)),
                            ('d', d, F.conv2d(x, wpj.double(), bpj.double(), stride=2))):
        mx, gate = err(got.view(b, ho, wo, cout).permute(0, 3, 1, 2), want)[0], 4e-6 * scale_of(want)
        record('6 entry kernel', f'{b}x{cin}x{h}x{w} -> {cout}, {name}', 'inside', 'conv_generic (entry)', mx, gate, cus)
        assert mx < gate, name


# ================================================================== row 7: the two-pass statistics merge of the NHWC norm
# nhwc_ops.hip:86-87 -- up to 32 x 32 = 1024 parts of 256 pixels stay in registers between the two sums; beyond, they are read twice.
@pytest.mark.parametrize('hw', [(512, 512), (513, 512)])
def test_norm_merge_at_1024_parts(ops, cus, hw):
    h, w = hw
    b, c = 1, 8
    parts = (h * w + db.NORM_CHUNK_ROWS - 1) // db.NORM_CHUNK_ROWS
    assert parts == (1024 if h == 512 else 1026)
    x = rnd(93, b, c, h, w, scale=2.0) + 30.0 * rnd(94, 1, c, 1, 1)         # a large mean: the shifted statistics
    _, xf = ops.nchw_to_nhwc(x.to(DEV).contiguous(), want_planes=False, want_f32=True)
    want = F.instance_norm(x.double())
    _, f32 = ops.nhwc_norm(xf, b, h * w, relu=False, want_planes=False, want_f32=True)
    mx = err(f32.view(b, h, w, c).permute(0, 3, 1, 2), want)[0]
    record('7 norm merge', f'{b}x{c}x{h}x{w}', f'{parts} parts ' + ('in registers' if parts <= db.NORM_PARTS_IN_REGISTERS else 'read twice'),
           'nhwc_stats_finalize_kernel', mx, 2e-5, cus)
    assert mx < 2e-5


# ================================================================== rows 8 .. 11: the multi-view plane sweeps (csrc/depth_multi.hip)
# um_depth_corr_softmax_multi and um_depth_corr_softmax_multi_rows pick depth_multi{,_rows}_box_kernel | _gather_kernel by
# ``num_candidates <= 64`` (depth_multi.hip:679, :746) and size their grid with pixel_grid_blocks (local_pixel.h:105).  No census id
# exists for them: the kernel of a record line is what that rule gives for the row's D.  Reference, inputs and gates are those of
# tests/test_depth_multiview_gpu.py (mv.reference_of in float64 on the float32 inputs, mv.compare through mv.compare_about_best); every record line names the float
# plane that came nearest its gate.  The properties of the inputs that make these cases able to fail, and three seeded defects that
# mv.compare rejects, are in tests/test_dispatch_boundaries_cpu.py.
def multi_kernel(d, launch):
    return ('depth_multi_rows_' if launch == 'rows' else 'depth_multi_') + ('box' if db.depth_uses_box_kernel(d) else 'gather') + '_kernel'


def check_multi(row, label, side, got, ref, d, cand, argmax, launch, cus):
    """One launch's ``(out, stats, index)`` through mv.compare_about_best (mv.compare, with the float64 ``peak_mass`` taken about the
    launch's own ``best``: on maps of this size the top two logits of a pixel can tie within fp32 rounding); with ``argmax`` the read-out
    must be the candidate at ``best``, which mv.compare then gates (the rule of test_against_float64)."""
    if argmax:
        assert torch.equal(got[0][:, 0], cand[got[2][:, 0].long()])
        ref = dict(ref, out=got[0].cpu().double())
    dist = mv.compare_about_best(got, ref, d, f'{label} {launch}')
    sc = mv.scales(d)
    plane = max(dist, key=lambda k: dist[k] / sc[k])
    record(row, f'{label}, {launch} launch, {plane}', side, multi_kernel(d, launch), dist[plane], mv.TOL * sc[plane], cus)


def run_multi_case(ops, cus, row, name, variant, side):
    """A BOUNDARY case of tests/depth_multiview_util.py on both launches: the contiguous one and the rows launch on the same operands
    scattered into four segments (``variant`` 'use': the mask of mv.boundary_geometry on the contiguous launch, one bad row index per off
    source on the rows launch).  The two agree bit for bit and each passes mv.compare against float64 on its own."""
    masked, argmax = variant == 'use', variant == 'argmax'
    (b, h, w), d, moves, use = mv.boundary_geometry(name, masked)
    f0, f1, cam, cand, use = mv.boundary_inputs(name, masked)
    ref = mv.boundary_reference(name, masked)
    segs, table, rows = fu.scatter(f0, f1, cam, 4, seed=len(name))
    if masked:
        bad = fu.switch_off(rows, use, sum(t.shape[0] for t in segs), table.shape[0], shift=len(moves))
        assert int((bad != rows).any(-1).sum()) == int((use == 0).sum()) > 0
        rows = bad
    cand_d = cand.to(DEV)
    whole = ops.depth_corr_softmax(f0.to(DEV), f1.to(DEV), h, w, cam.to(DEV), cand_d, argmax, stats=True,
                                   use=use.to(DEV) if masked else None)
    by_rows = ops.depth_corr_softmax([t.to(DEV) for t in segs], None, h, w, table.to(DEV), cand_d, argmax, stats=True, rows=rows.to(DEV))
    assert tuple(whole[0].shape) == (b, 1, h, w) and tuple(whole[1].shape) == (b, 4, h, w) and tuple(whole[2].shape) == (b, 2, h, w)
    for what, a, e in zip(('out', 'stats', 'index'), by_rows, whole):
        assert a.dtype == e.dtype and torch.equal(a, e), (name, variant, what, (a.double() - e.double()).abs().max().item())
    for launch, got in (('contiguous', whole), ('rows', by_rows)):
        check_multi(row, f'{name} S={len(moves)} {variant}', side, got, ref, d, cand_d, argmax, launch, cus)


# ------------------------------------------------------------------ row 8: past the grid cap, all four kernels
# local_pixel.h:105-110 -- past 16384 pixels a wave goes round ``pid += gridDim.x * 4`` again and reuses its LDS table, the `gathered`
# flag and acc / cnt (depth_multi.hip:216, :353, :463, :600).  128 x 128 is the last one-trip map; 129 x 128 sends 32 workgroups round
# again; at 2 x 91 x 91 sample 1 starts at pixel 8281, inside a workgroup, and 178 pixels are on the second trip.
@pytest.mark.parametrize('variant', ['soft', 'argmax', 'use'])
@pytest.mark.parametrize('name', [n for n in mv.BOUNDARY if n.startswith('cap-')])
def test_grid_cap_multi_view_sweep(ops, cus, name, variant):
    (b, h, w), d, moves = mv.BOUNDARY[name]
    trips = db.pixel_grid_trips(b * h * w)
    assert trips == (1 if b * h * w <= mv.GRID_PIXELS else 2) and int(mv.second_trip(b, h, w).sum()) == max(0, b * h * w - mv.GRID_PIXELS)
    run_multi_case(ops, cus, '8 grid cap, multi-view sweep', name, variant, f'{trips} trip(s)')


# ------------------------------------------------------------------ row 9: four to eight sources
# The ABI takes S = 1 .. 8 (depth_multi.hip:665, :710): eight sources of which up to seven see a candidate, and five; under 'use' three
# samples keep 1, 4 and 7 (of five: 5) sources.
@pytest.mark.parametrize('variant', ['soft', 'use'])
@pytest.mark.parametrize('name', [n for n in mv.BOUNDARY if n.startswith(('s8-', 's5-'))])
def test_source_count_multi_view_sweep(ops, cus, name, variant):
    (b, h, w), d, moves, use = mv.boundary_geometry(name, variant == 'use')
    on = 'every source on' if use is None else 'sources on per sample ' + ' / '.join(str(int(n)) for n in use.sum(0))
    run_multi_case(ops, cus, '9 source count, multi-view sweep', name, variant, f'{len(moves)} of 8 sources, {on}')


def test_nine_sources_are_refused_by_both_entry_points(lib, cus):
    """``sources = 9``: UM_ERR_UNSUPPORTED with a message from um_depth_corr_softmax_multi and um_depth_corr_softmax_multi_rows, the
    output untouched (nothing was launched); eight sources on the same buffers are served."""
    import ctypes
    b, h, w, d = 1, 4, 5, 16
    moves = mv.EIGHT + ('sideways',)
    f0, f1 = (t.to(DEV) for t in mv.features(b, h, w, moves))
    cam, cand = mv.cameras(b, h, w, moves).to(DEV), mv.candidates(d).to(DEV)
    rows = torch.arange(9 * b, dtype=torch.int32).view(9, b, 1).repeat(1, 1, 3)
    rows[..., 1] += 9 * b
    rows = rows.to(DEV).contiguous()
    tokens, table = torch.cat([f0.flatten(0, 1), f1.flatten(0, 1)], 0).contiguous(), cam.flatten(0, 1).contiguous()
    ptrs, counts = (ctypes.c_void_p * 1)(tokens.data_ptr()), (ctypes.c_int * 1)(tokens.shape[0])
    out = torch.full((b, 1, h, w), -7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    calls = {
        'um_depth_corr_softmax_multi': lambda s: lib.um_depth_corr_softmax_multi(p(f0), p(f1), p(cam), None, p(cand), p(out), None, None, s, b,
                                                                                 h, w, C, d, 0, 1, st),
        'um_depth_corr_softmax_multi_rows': lambda s: lib.um_depth_corr_softmax_multi_rows(ptrs, counts, 1, p(table), table.shape[0], p(rows),
                                                                                           p(cand), p(out), None, None, s, b, h, w, C, d, 0, 1, st),
    }
    for what, call in calls.items():
        rc = call(9)
        assert rc == db.UM_ERR_UNSUPPORTED and b'sources=9' in lib.um_last_error_string(), (what, rc)
        torch.cuda.synchronize()
        assert bool((out == -7).all()), what
        record('9 refusals', f'{what}, 9 sources', 'one step beyond', f'refused ({rc})', 0.0, 0.0, cus)
    want = None
    for what, call in calls.items():
        out.fill_(-7.0)
        assert call(8) == 0, what
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and bool((out != -7).all()), what
        want = out.clone() if want is None else want
        assert torch.equal(out, want)                                                # the table names the same operands in order


# ------------------------------------------------------------------ row 10: the fourth segment and the segment edges
# DepthSegments has four pointers (depth_multi.hip:416-431).  fu.scatter_edges: segments of 1, n, 1, m rows whose first and last rows
# are all named, row ``total - 1`` and the off index ``total`` in neighbouring entries.  (Four shuffled segments at every case:
# test_rows_launch_is_the_contiguous_launch of tests/test_depth_fuse_neighbours_gpu.py, and rows 8 and 9 above.)
@pytest.mark.parametrize('argmax', [False, True])
@pytest.mark.parametrize('case', ['B', 'C'])
def test_segment_edges_and_the_fourth_segment(ops, cus, case, argmax):
    (b, h, w), d, moves = mv.CASES[case]
    f0, f1, cam, cand = mv.inputs(case)
    segs, table, rows, use, ref = fu.edges_case(case)
    total = sum(t.shape[0] for t in segs)
    assert len(segs) == 4 and segs[0].shape[0] == segs[2].shape[0] == 1 and int(rows[..., :2].max()) == total
    cand_d = cand.to(DEV)
    whole = ops.depth_corr_softmax(f0.to(DEV), f1.to(DEV), h, w, cam.to(DEV), cand_d, argmax, stats=True, use=use.to(DEV))
    by_rows = ops.depth_corr_softmax([t.to(DEV) for t in segs], None, h, w, table.to(DEV), cand_d, argmax, stats=True, rows=rows.to(DEV))
    for what, a, e in zip(('out', 'stats', 'index'), by_rows, whole):
        assert a.dtype == e.dtype and torch.equal(a, e), (case, what, (a.double() - e.double()).abs().max().item())
    sizes = ' + '.join(str(t.shape[0]) for t in segs)
    check_multi('10 segment edges, rows launch', f'case {case} {"argmax" if argmax else "soft"}, segments of {sizes} rows',
                'first and last row of 4 segments', by_rows, ref, d, cand_d, argmax, 'rows', cus)


# ------------------------------------------------------------------ row 11: every round of the gather form, sources that differ
# acc[8] / cnt[8] of depth_multi_gather_kernel (depth_multi.hip:356-391): 96 candidates are six whole rounds, 113 one candidate past
# seven, 128 the limit -- with three different sources, so that a count gone wrong in rounds 5 .. 7 does not cancel.
@pytest.mark.parametrize('name', [n for n in mv.BOUNDARY if n.startswith('rounds-')])
def test_gather_rounds_with_sources_that_differ(ops, cus, name):
    (b, h, w), d, moves = mv.BOUNDARY[name]
    f0, f1, cam, cand, _ = (t if t is None else t.to(DEV) for t in mv.boundary_inputs(name))
    ref = mv.boundary_reference(name)
    row, side = '11 gather rounds, sources that differ', f'{(d + 15) // 16} rounds, {d} of 128'
    for argmax in (False, True):
        got = ops.depth_corr_softmax(f0, f1, h, w, cam, cand, argmax, stats=True)
        check_multi(row, f'{name} S={len(moves)} {"argmax" if argmax else "soft"}', side, got, ref, d, cand, argmax, 'contiguous', cus)
    _, stats, _ = ops.depth_corr_softmax(f0, f1, h, w, cam, cand, stats=True, peak_radius=0)
    off = (stats[:, 3].double() - stats[:, 0].double()).abs().max().item()
    record(row, f'{name} peak_radius 0, peak_mass against max_prob', side, multi_kernel(d, 'contiguous'), off, mv.TOL, cus)
    assert off <= mv.TOL
    assert (stats[:, 0].cpu().double() - ref['stats'].max_prob).abs().max().item() <= mv.TOL
    _, stats, _ = ops.depth_corr_softmax(f0, f1, h, w, cam, cand, stats=True, peak_radius=d)
    off = (stats[:, 3].double() - 1.0).abs().max().item()
    record(row, f'{name} peak_radius {d}, peak_mass against 1', side, multi_kernel(d, 'contiguous'), off, 1e-6, cus)
    assert off <= 1e-6
