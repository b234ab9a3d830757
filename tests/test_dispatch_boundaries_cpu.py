"""The host side of the kernel-selection rules, without a GPU: the exported plan / split / part-count functions on both sides of every
switch, the Python restatements tests/dispatch_boundaries.py uses against the library's answers, the refusals one step beyond the
advertised tap and candidate range (decided on the host before any HIP call), the conditioning of the arg-max read-out's inputs, and
(at the end) the properties of the multi-view sweeps' inputs of rows 8 .. 11 with three seeded defects that their gate rejects.
Without a device the library's CU count is its fallback of 256 (common.h:19-28); every assertion below holds for any count."""
import ctypes

import pytest
import torch

from tests import depth_fuse_neighbours_util as fu
from tests import depth_multiview_util as mv
from tests import dispatch_boundaries as db
from unimatch_amd import _abi, confidence


@pytest.fixture(scope='module')
def lib():
    return _abi.load()


def _cus(lib):
    """The CU count the plan functions use, recovered from the FFN rule: the largest tile count that still splits in two is CUs / 2."""
    steps = db.ffn_split_steps(lib, 1024)
    assert steps and steps[-1][2:] == (2, 1), steps
    return 2 * (steps[-1][0] // 128)


# ------------------------------------------------------------------ window attention: token table and key split
def test_token_table_holds_windows_of_2048_tokens():
    """window_attn.hip:231.  The geometries of row 1 of the GPU file sit where they are meant to."""
    assert db.attn_uses_token_table(32, 64) and not db.attn_uses_token_table(1, 2080) and not db.attn_uses_token_table(40, 52)
    assert not db.attn_uses_token_table(33, 64) and db.attn_uses_token_table(1, 2048) and not db.attn_uses_token_table(1, 2049)


def test_key_split_needs_eight_and_sixteen_key_tiles(lib):
    """window_attn.hip:1100 -- ``ntiles >= 4 * (2 * split)``: one window of 7 key tiles (224 tokens) stays whole, 8 (256 tokens) splits in
    two, 15 (480) stays at two, 16 (512) splits in four -- on any device with at least 16 CUs."""
    assert db.attn_plan(lib, 1, 14, 16, 14, 16) == (2, 0, 1)
    assert db.attn_plan(lib, 1, 16, 16, 16, 16) == (0, 2, 2)
    assert db.attn_plan(lib, 1, 15, 32, 15, 32) == (0, 4, 2)
    assert db.attn_plan(lib, 1, 16, 32, 16, 32) == (0, 4, 4)
    assert lib.um_window_attn_ksplit_workspace_bytes(1, 14, 16, 14, 16) == 0
    assert lib.um_window_attn_ksplit_workspace_bytes(1, 16, 16, 16, 16) == 256 + 2 * 2 * 17 * 256 * 4 * 4     # window_attn.hip:1132


def test_key_split_steps_follow_the_cu_count(lib):
    """window_attn.hip:1100, 1125 -- ``total * 2 * split <= 2 * CUs``: stacking 512-token windows, the launch goes from 4 parts to 2
    when its tiles pass CUs / 2 and from 2 to 1 when they pass CUs, and the restated rule agrees with the library at every count."""
    cus = _cus(lib)
    steps = db.attn_split_steps(lib)
    assert [s[2:] for s in steps] == [(4, 2), (2, 1)], steps
    assert 4 * steps[0][0] <= cus // 2 < 4 * steps[0][1] and 4 * steps[1][0] <= cus < 4 * steps[1][1], (steps, cus)
    wh, ww = db.STEP_WINDOW
    for k in range(1, 200):
        assert db.attn_parts(lib, 1, wh * k, ww, wh, ww) == db.attn_split_rule(4 * k, 16, cus), k
    # the 2112-token shifted geometry of row 1: 17 query tiles x 4 windows, 66 key tiles
    for s in (1, 2, 3, 4, 8):
        assert db.attn_parts(lib, s, 66, 128, 33, 64) == db.attn_split_rule(68 * s, 66, cus), s
    assert db.attn_parts(lib, db.attn_unsplit_streams(lib, 66, 128, 33, 64), 66, 128, 33, 64) == 1


def test_plan_rejects_bad_geometry(lib):
    f = ctypes.c_int()
    assert lib.um_window_attn_plan(1, 10, 10, 3, 5, ctypes.byref(f), ctypes.byref(f), ctypes.byref(f)) == db.UM_ERR_BAD_ARG
    assert lib.um_window_attn_plan(1, 10, 10, 5, 5, None, ctypes.byref(f), ctypes.byref(f)) == db.UM_ERR_BAD_ARG
    assert lib.um_window_attn_ksplit_workspace_bytes(1, 10, 10, 3, 5) == 0


# ------------------------------------------------------------------ FFN hidden split
def test_ffn_split_steps_follow_the_cu_count(lib):
    """ffn.hip:983 -- ``tiles * 2 * split <= CUs`` at hidden 1024 (32 slices: no slice condition binds): 4 parts up to CUs / 4 tiles,
    2 up to CUs / 2, then none; the byte count is the closed form of ffn.hip:987-990."""
    cus = _cus(lib)
    steps = db.ffn_split_steps(lib, 1024)
    assert [s[2:] for s in steps] == [(4, 2), (2, 1)], steps
    assert steps[0][0] == 128 * (cus // 4) and steps[1][0] == 128 * (cus // 2), (steps, cus)
    for m in (1, 128, 129, steps[0][0], steps[0][1], steps[1][0], steps[1][1], 100000):
        assert db.ffn_split(lib, m, 1024) == db.ffn_split_rule(m, 1024, cus), m
    if cus == 256:
        assert [s[:2] for s in steps] == [(8192, 8193), (16384, 16385)]
    m = steps[0][0]
    assert lib.um_ffn_split_workspace_bytes(m, 1024) == (m // 128 * 4 + 255) // 256 * 256 + m // 128 * 4 * 64 * 256 * 4


def test_ffn_split_slice_conditions(lib):
    """ffn.hip:983 -- ``nslice % (2 * split) == 0 && nslice / (2 * split) >= 4`` at one tile: 2, 3 and 4 slices do not split, 8 split in
    two (4 per part; 2 per part would be too few for four), 10 split in two (an odd 5 per part cannot halve again), 16 split in four."""
    want = {64: 1, 96: 1, 128: 1, 224: 1, 256: 2, 320: 2, 384: 2, 512: 4, 1024: 4}
    cus = _cus(lib)
    for hidden, split in want.items():
        assert db.ffn_split(lib, 128, hidden) == split == db.ffn_split_rule(128, hidden, cus), hidden
    assert lib.um_ffn_split_workspace_bytes(128, 48) == 0 and lib.um_ffn_split_workspace_bytes(0, 1024) == 0      # not served at all


# ------------------------------------------------------------------ local family: grid cap, tap range, refusals
def test_pixel_grid_cap_is_16384_pixels():
    """local_pixel.h:105-110."""
    assert db.pixel_grid_trips(128 * 128) == 1 and db.pixel_grid_trips(129 * 128) == 2 and db.pixel_grid_trips(1) == 1
    assert db.pixel_grid_trips((2 * 363 * 362 + 15) // 16) == 2 and db.pixel_grid_trips(262144 // 16) == 1   # K4: blocks of 16 pixels


def _buffers():
    """Pointers for calls that must be refused before any HIP call.  Without a device they are fake and non-null -- a call that was
    let through returns a positive HIP error.  With a device they are real and large enough for the geometry asked for, so that a
    call that was let through is a failed assertion and nothing else."""
    if torch.cuda.is_available():
        keep = [torch.zeros(1 << 18, dtype=torch.float32, device='cuda') for _ in range(7)]
        return keep, [t.data_ptr() for t in keep]
    return None, [0x1000 * (i + 1) for i in range(7)]


def test_refusals_beyond_the_tap_range_are_decided_on_the_host(lib):
    """One step beyond LOCAL_MAX_ROUNDS x 16 = 128 taps / candidates (local_ops.hip:673, 792, 806, 831) and beyond the cost volume's 81
    taps (:691, :774): UM_ERR_UNSUPPORTED and a message, on 8 x 8 maps."""
    keep, (a, b, c, d, e, f, g) = _buffers()
    lib.um_census_enable(1)
    calls = {
        '2-D radius 6 (169 taps)': lambda: lib.um_local_corr_softmax(a, b, c, 1, 8, 8, 128, 6, 0, None),
        '1-D radius 64 (129 taps)': lambda: lib.um_local_corr_softmax(a, b, c, 1, 8, 8, 128, 64, 1, None),
        'prop_local radius 6': lambda: lib.um_prop_local_attn(a, b, c, d, 1, 8, 8, 128, 2, 6, None),
        '129 candidates': lambda: lib.um_depth_corr_softmax(a, b, c, d, e, 1, 8, 8, 128, 129, 0, None),
        '129 candidates, stats': lambda: lib.um_depth_corr_softmax_stats(a, b, c, d, e, f, g, 1, 8, 8, 128, 129, 0, 1, None),
        'no candidate': lambda: lib.um_depth_corr_softmax(a, b, c, d, e, 1, 8, 8, 128, 0, 0, None),
        'cost volume radius 5 (121 taps)': lambda: lib.um_local_corr_with_flow(a, b, c, d, 1, 8, 8, 128, 5, None),
        'dilated cost volume radius 5': lambda: lib.um_local_corr_with_flow_dilated(a, b, c, d, 1, 8, 8, 128, 5, 2, None),
    }
    for what, call in calls.items():
        rc = call()
        assert rc == db.UM_ERR_UNSUPPORTED, (what, rc)
        assert lib.um_last_error_string(), what
    assert all(v == 0 for v in _abi.census(lib).values())                  # no launch was counted
    lib.um_census_enable(0)
    del keep


def test_the_last_served_tap_counts():
    """What row 5 of the GPU file runs is inside the range: 2-D radius 5 = 121 taps, 1-D radius 63 = 127, 128 candidates."""
    assert 11 * 11 <= db.LOCAL_MAX_TAPS < 13 * 13 and 2 * 63 + 1 <= db.LOCAL_MAX_TAPS < 2 * 64 + 1
    assert 9 * 9 <= db.K4_MAX_TAPS < 11 * 11
    assert db.depth_uses_box_kernel(64) and not db.depth_uses_box_kernel(65)


@pytest.mark.parametrize('nd', db.SWEEP_COUNTS)
def test_argmax_inputs_are_well_conditioned_in_fp32(nd):
    """The arg-max read-out is gated by "at most 1 % of the pixels differ by more than 1e-6" from the fp64 oracle.  That gate is only
    fair where fp32 arithmetic itself decides the arg-max as fp64 does: for the candidates and features of row 5, the fp32 evaluation
    of the same oracle stays within that 1 %."""
    b, h, w = db.SWEEP_SMALL
    want = db.sweep_reference(b, h, w, nd, True)
    f32 = db.sweep_reference(b, h, w, nd, True, torch.float32)
    differ = (f32.double() - want).abs().gt(1e-6).float().mean().item()
    assert differ < 0.01, (nd, differ)


# ------------------------------------------------------------------ conv_pick
PICK = [
    # hi, wi, cout, kh, kw, stride, ph, pw -> kind            conv.hip:1199: the row-window kernel needs ho * wo >= 256
    ((15, 17, 64, 3, 3, 1, 1, 1), 'generic'), ((16, 16, 64, 3, 3, 1, 1, 1), 'rows'),
    # conv.hip:1203: the patch kernel needs 4 ho wo >= 3 x the area of its 8 x 32 tiles
    ((17, 33, 64, 3, 3, 1, 1, 1), 'rows'), ((24, 32, 64, 3, 3, 1, 1, 1), 'patch'),
    ((5, 64, 64, 3, 3, 1, 1, 1), 'rows'), ((6, 64, 64, 3, 3, 1, 1, 1), 'patch'),          # ragged in rows only: 5/8 | 6/8 of a tile
    ((8, 47, 64, 3, 3, 1, 1, 1), 'rows'), ((8, 48, 64, 3, 3, 1, 1, 1), 'patch'),          # ragged in columns only: 47/64 | 48/64
    # conv.hip:1200: five-tap rows on 128-wide tiles only
    ((16, 16, 128, 1, 5, 1, 0, 2), 'rows'), ((16, 16, 96, 1, 5, 1, 0, 2), 'generic'),
    ((16, 16, 128, 5, 1, 1, 2, 0), 'generic'), ((16, 16, 96, 5, 1, 1, 2, 0), 'generic'),
    ((16, 32, 64, 3, 3, 2, 1, 1), 'generic'), ((16, 32, 64, 3, 3, 1, 0, 0), 'generic'),
]
WIDTHS = {4: 2, 32: 2, 36: 2, 64: 2, 96: 3, 128: 4, 160: 4, 192: 3, 200: 4, 256: 4}           # conv.hip:1191


def test_conv_pick_restated_agrees_with_the_library(lib):
    """conv.hip:1189-1250.  um_conv_stats_parts and um_conv2d_norm_supported are the library's own reading of conv_pick: the part count
    is the patch kernel's ``2 x tiles`` exactly where the restated rule says 'patch', and the on-load kernel is offered there and only
    there (for tile widths of at least 64 columns)."""
    for geo, kind in PICK:
        hi, wi, cout, kh, kw, stride, ph, pw = geo
        got, nt = db.conv_kind(*geo)
        assert got == kind, (geo, got)
        ho, wo = (hi + 2 * ph - kh) // stride + 1, (wi + 2 * pw - kw) // stride + 1
        assert lib.um_conv_stats_parts(*geo) == db.conv_parts(kind, ho, wo), geo
        assert lib.um_conv2d_norm_supported(hi, wi, 64, cout, kh, kw, stride, ph, pw, 0) == int(kind == 'patch'), geo
    assert {c: db.conv_tile_width(c) for c in WIDTHS} == WIDTHS
    for cout, nt in WIDTHS.items():
        assert db.conv_kind(16, 32, cout, 3, 3, 1, 1, 1) == ('patch', 1 if cout <= 32 else nt)
        assert db.conv_kind(9, 11, cout, 3, 3, 1, 1, 1) == ('generic', nt)
        # conv.hip:1205, 1224: a head of up to 32 outputs takes the 32-wide tile, which has no on-load form
        assert lib.um_conv2d_norm_supported(16, 32, 64, cout, 3, 3, 1, 1, 1, 0) == int(cout > 32), cout
        assert lib.um_conv2d_norm_supported(9, 11, 64, cout, 3, 3, 1, 1, 1, 0) == 0
    # the 3/4 rule tells the two part counts apart wherever they differ: the sweep of every size up to 40 x 70
    for hi in range(1, 41):
        for wi in range(1, 71):
            kind, _ = db.conv_kind(hi, wi, 64, 3, 3, 1, 1, 1)
            assert lib.um_conv_stats_parts(hi, wi, 64, 3, 3, 1, 1, 1) == db.conv_parts(kind, hi, wi), (hi, wi)
            assert lib.um_conv2d_norm_supported(hi, wi, 64, 64, 3, 3, 1, 1, 1, 0) == int(kind == 'patch'), (hi, wi)


def test_entry_kernel_conditions(lib):
    """conv.hip:1232-1241: 3x3 / stride 2 / pad 1, at most 128 input channels, 96- and 128-wide output tiles."""
    ok = lib.um_conv2d_entry_supported
    assert ok(17, 33, 128, 128, 3, 3, 2, 1, 1, 0) == 1 and ok(17, 33, 160, 128, 3, 3, 2, 1, 1, 0) == 0       # cin 128 | 160
    assert ok(17, 33, 64, 96, 3, 3, 2, 1, 1, 0) == 1 and ok(17, 33, 64, 64, 3, 3, 2, 1, 1, 0) == 0           # NT 3 | 2
    assert ok(17, 33, 96, 192, 3, 3, 2, 1, 1, 0) == 1 and ok(17, 33, 96, 200, 3, 3, 2, 1, 1, 0) == 1         # NT 3 | 4
    assert ok(17, 33, 64, 96, 3, 3, 1, 1, 1, 0) == 0 and ok(17, 33, 64, 96, 5, 5, 2, 2, 2, 0) == 0
    assert ok(17, 33, 64, 96, 3, 3, 2, 0, 0, 0) == 0 and ok(17, 33, 48, 96, 3, 3, 2, 1, 1, 0) == 0


def test_convolution_refuses_two_output_channels_on_the_host(lib):
    """The flow head's 256 -> 2 is served as a convolution padded to 4 outputs: ``cout % 4 != 0`` is a bad argument (conv.hip:1268)."""
    keep, (a, b, c, d, e, f, g) = _buffers()
    rc = lib.um_conv2d_fwd(a, b, None, c, None, 1, 8, 8, 32, 2, 3, 3, 1, 1, 1, 0, 10, 0, None)
    assert rc == db.UM_ERR_BAD_ARG and lib.um_last_error_string()
    del keep


# ------------------------------------------------------------------ NHWC norm
def test_norm_statistics_parts_of_the_gpu_rows():
    """nhwc_ops.hip:15, 86-87: chunks of 256 pixels; up to 1024 parts stay in registers."""
    assert 512 * 512 // db.NORM_CHUNK_ROWS == db.NORM_PARTS_IN_REGISTERS and 513 * 512 // db.NORM_CHUNK_ROWS == db.NORM_PARTS_IN_REGISTERS + 2


# ------------------------------------------------------------------ rows 8 .. 11: the multi-view plane sweeps, on the reference alone
# What the inputs of rows 8 .. 11 of the GPU file must be for those rows to be able to fail, asserted on the float64 reference; the
# host twin of the segment-edge table; and three seeded defects that mv.compare rejects at the row that targets each.
def test_multi_view_cap_geometries_sit_where_they_are_meant_to():
    """local_pixel.h:105-110: 16384 pixels are the last one-trip map; 129 x 128 sends 32 workgroups round again; at 2 x 91 x 91 sample 1
    starts inside a workgroup and 178 pixels are on the second trip."""
    assert db.PIXEL_GRID_CAP * 4 == mv.GRID_PIXELS == 16384
    assert [db.pixel_grid_trips(b * h * w) for b, h, w in ((1, 128, 128), (1, 129, 128), (2, 91, 91))] == [1, 2, 2]
    assert int(mv.second_trip(1, 128, 128).sum()) == 0 and int(mv.second_trip(1, 129, 128).sum()) == 128 == 32 * 4
    trip = mv.second_trip(2, 91, 91)
    assert int(trip.sum()) == 178 and not bool(trip[0].any()) and 91 * 91 == 8281 and 8281 % 4 != 0
    assert {mv.BOUNDARY[n][1] for n in mv.BOUNDARY if n.startswith('cap-')} == {16, 65}
    assert db.depth_uses_box_kernel(16) and not db.depth_uses_box_kernel(65)


@pytest.mark.parametrize('name', [n for n in mv.BOUNDARY if n.startswith('cap-')])
def test_multi_view_cap_inputs_cannot_go_soft(name):
    """Row 8.  On the whole map: ``clear`` covers at least 0.90 and the largest |logit| exceeds 9 (the softmax is not flat).  On the
    second trip (``pid >= 16384``): by mv.box_positions at least one source takes the box form and at least one the gather form, at
    least 5 % of the (pixel, candidate) pairs have n_j = 1 and at least 15 % have n_j >= 2 -- a table, a `gathered` flag or a count
    carried over from the first trip changes the result."""
    (b, h, w), d, moves = mv.BOUNDARY[name]
    ref = mv.boundary_reference(name)
    clear, peak = ref['clear'].float().mean().item(), ref['logits'].abs().max().item()
    print(f'{name}: clear {clear:.4f} |logit|max {peak:.2f}')
    assert clear >= 0.90 and peak > 9, (name, clear, peak)
    masked = mv.boundary_reference(name, True)
    assert masked['clear'].float().mean().item() >= 0.90
    assert (masked['out'][b - 1] - ref['out'][b - 1]).abs().max().item() > 2e-3          # the source that is off had a say
    trip = mv.second_trip(b, h, w)
    if not bool(trip.any()):
        return
    box = {m: (mv.box_positions(h, w, mv.camera(b, h, w, m), mv.candidates(d))[trip] <= mv.DEPTH_BOX).double().mean().item() for m in moves}
    views = ref['views'].permute(0, 2, 3, 1)[trip]
    share = [(views == n).double().mean().item() for n in range(len(moves) + 1)]
    print(f'{name}: second trip, box form ' + ' '.join(f'{m} {v:.3f}' for m, v in box.items()) + ' | n_j = 0 | 1 | 2 | 3: '
          + ' | '.join(f'{v:.3f}' for v in share))
    assert any(v > 0 for v in box.values()) and any(v < 1 for v in box.values()), box
    assert share[1] >= 0.05 and sum(share[2:]) >= 0.15, share


@pytest.mark.parametrize('name', [n for n in mv.BOUNDARY if n.startswith(('s8-', 's5-'))])
def test_multi_view_source_count_inputs(name):
    """Row 9.  Eight sources: n_j takes each of the values 4, 5, 6 and 7 on at least 1 % of the (pixel, candidate) pairs and never less
    than 4; five sources: 2, 3 and 4.  Under the mask the three samples keep 1, 4 and 7 (of five: 5) sources, each sample's result
    differs from the unmasked sweep's, and ``clear`` covers at least 0.90 both times."""
    (b, h, w), d, moves = mv.BOUNDARY[name]
    s = len(moves)
    ref = mv.boundary_reference(name)
    share = [(ref['views'] == n).double().mean().item() for n in range(s + 1)]
    print(f'{name}: n_j = 0 .. {s}: ' + ' | '.join(f'{v:.3f}' for v in share) + f' clear {ref["clear"].float().mean().item():.4f}')
    top = s - 1                                                  # 'away' sees nothing
    assert all(v >= 0.01 for v in share[top - (3 if s == 8 else 2):top + 1]) and share[s] == 0, share
    assert sum(share[:top - (3 if s == 8 else 2)]) == 0, share
    assert ref['clear'].float().mean().item() >= 0.90 and ref['logits'].abs().max().item() > 9
    (mb, _, _), _, _, use = mv.boundary_geometry(name, True)
    assert mb == 3 and use.sum(0).tolist() == [1, 4, min(7, s)]
    masked = mv.boundary_reference(name, True)
    assert masked['clear'].float().mean().item() >= 0.90
    assert [int(masked['views'][i].max()) for i in range(3)] == [1, 4 - int(use[4, 1]), min(7, s) - int(use[4, 2])]
    whole = mv.reference_of(*mv.boundary_inputs(name, True)[:2], h, w, *mv.boundary_inputs(name, True)[2:4])
    for i in range(3 if s == 8 else 2):
        assert (masked['out'][i] - whole['out'][i]).abs().max().item() > 2e-3, i


@pytest.mark.parametrize('name', [n for n in mv.BOUNDARY if n.startswith('rounds-')])
def test_multi_view_upper_round_inputs(name):
    """Row 11.  Among the candidates of rounds 5 .. 7 of the gather form (index 80 and beyond) at least 15 % of the (pixel, candidate)
    pairs are seen by two or more sources and at least two different counts n_j >= 1 occur on 5 % each: a count that goes wrong there does
    not cancel.  ``clear`` covers at least 0.90."""
    (b, h, w), d, moves = mv.BOUNDARY[name]
    ref = mv.boundary_reference(name)
    upper = ref['views'][:, 80:]
    share = [(upper == n).double().mean().item() for n in range(len(moves) + 1)]
    print(f'{name}: candidates 80 .. {d - 1}: n_j = 0 | 1 | 2 | 3: ' + ' | '.join(f'{v:.3f}' for v in share)
          + f' clear {ref["clear"].float().mean().item():.4f}')
    assert d > 80 and (d + 15) // 16 >= 6
    assert sum(share[2:]) >= 0.15 and sum(v >= 0.05 for v in share[1:]) >= 2, share
    assert ref['clear'].float().mean().item() >= 0.90 and ref['logits'].abs().max().item() > 9


def test_nine_sources_are_refused_on_the_host_by_both_entry_points(lib):
    """depth_multi.hip:665, :710 -- ``sources`` 1 .. 8; 0 and 9 are UM_ERR_UNSUPPORTED from um_depth_corr_softmax_multi and from
    um_depth_corr_softmax_multi_rows, decided before any HIP call."""
    keep, (a, b, c, d, e, f, g) = _buffers()
    ptrs, counts = (ctypes.c_void_p * 1)(a), (ctypes.c_int * 1)(64)
    for sources in (0, 9):
        rc = lib.um_depth_corr_softmax_multi(a, b, c, None, d, e, f, g, sources, 1, 8, 8, 128, 16, 0, 1, None)
        assert rc == db.UM_ERR_UNSUPPORTED and f'sources={sources}'.encode() in lib.um_last_error_string(), (sources, rc)
        rc = lib.um_depth_corr_softmax_multi_rows(ptrs, counts, 1, c, 8, b, d, e, f, g, sources, 1, 8, 8, 128, 16, 0, 1, None)
        assert rc == db.UM_ERR_UNSUPPORTED and f'sources={sources}'.encode() in lib.um_last_error_string(), (sources, rc)
    del keep


@pytest.mark.parametrize('case', ['B', 'C'])
def test_segment_edge_table_names_what_it_was_made_from(case):
    """Row 10, host twin.  fu.scatter_edges: segments of 1, n, 1, m rows; the first and the last row of every segment are named by an
    entry that is on; ``total - 1`` and ``total`` are the f0 rows of neighbouring entries; depth_rows_to_source_major_host gives back
    the operands the table was made from and switches the entry with row ``total`` off."""
    (b, h, w), d, moves = mv.CASES[case]
    f0, f1, cam, cand = mv.inputs(case)
    segs, table, rows, use, ref = fu.edges_case(case)
    sizes = [t.shape[0] for t in segs]
    total = sum(sizes)
    assert len(segs) == 4 and sizes[0] == sizes[2] == 1 and sizes[1] >= 2 and sizes[3] >= 2
    first = [0, sizes[0], sizes[0] + sizes[1], total - sizes[3]]
    edges = set(first) | {f + n - 1 for f, n in zip(first, sizes)}
    named = set(rows[..., :2][use.bool()].flatten().tolist())
    assert len(edges) == 6 and edges <= named and len(named) == 2 * int(use.sum())             # no row is named twice
    flat = rows.view(-1, 3)
    k = flat[:, 0].tolist().index(total - 1)
    assert flat[k + 1, 0] == total and use.flatten().tolist()[k:k + 2] == [1, 0] and int((use == 0).sum()) == 1
    tokens = torch.cat(segs, 0)
    assert bool(torch.isnan(tokens).any()) and not bool(torch.isnan(tokens[sorted(named)]).any())
    g0, g1, gc, on = confidence.depth_rows_to_source_major_host(segs, table, rows)
    assert torch.equal(on, use.bool())
    assert torch.equal(g0[on], f0[on]) and torch.equal(g1[on], f1[on]) and torch.equal(gc[on], cam[on])
    logits, seen, views = confidence.depth_match_logits_multi_host([t.double() for t in segs], None, h, w, table.double(), cand.double(),
                                                                   rows=rows)
    assert torch.equal(logits, ref['logits']) and torch.equal(views, ref['views'])
    assert ref['clear'].float().mean().item() >= 0.90


def rejected(got, ref, d, label, gate=mv.compare_about_best):
    """Whether the gate of rows 8 .. 11 of the GPU file rejects ``got``."""
    try:
        gate(got, ref, d, label)
    except AssertionError:
        return True
    return False


def test_a_tie_of_the_top_two_logits_moves_peak_mass_and_nothing_else():
    """Why rows 8 .. 11 gate through mv.compare_about_best.  At 1 x 128 x 128 with D = 65 one pixel's top two float64 logits are less
    than 1e-5 apart (4.3e-6), closer than fp32 resolves at |logit| ~ 10.  A result that is the float64 one except that this pixel's
    ``best`` is the other candidate, with ``peak_mass`` about it, is as right as fp32 can be: mv.compare rejects it on ``peak_mass`` alone
    (the two windows differ by 1.8e-3, nine times the gate), mv.compare_about_best accepts it -- and rejects the same result when its
    ``peak_mass`` stays about the float64 ``best``, or when ``best`` moves at a pixel whose gap is not a tie."""
    name = 'cap-1x128x128-d65'
    (b, h, w), d, moves = mv.BOUNDARY[name]
    ref = mv.boundary_reference(name)
    gap = ref['gap']
    assert gap.min().item() < 1e-5 < mv.FLIP_GAP
    at = (gap == gap.min()).nonzero()[0]
    i, y, x = (int(v) for v in at)
    first, second = (int(v) for v in ref['prob'][i, :, y, x].topk(2)[1])
    about = ref['prob'][i, max(0, second - 1):second + 2, y, x].sum().item()
    moved = abs(about - ref['stats'].peak_mass[i, y, x].item())
    print(f'{name}: pixel ({y}, {x}) gap {gap.min().item():.2e}, best {first} | {second}, peak_mass windows differ by {moved:.3e}')
    assert moved > 5 * mv.TOL
    good = mv.result_of(ref)
    tied = tuple(t.clone() for t in good)
    tied[2][i, 0, y, x] = second
    assert rejected(tied, ref, d, 'tie, peak_mass about the float64 best')                      # best moved, peak_mass did not
    tied[1][i, 3, y, x] = about
    assert rejected(tied, ref, d, 'tie, plain compare', gate=mv.compare) and not rejected(tied, ref, d, 'tie, about its own best')
    wide = (gap > 1.0).nonzero()[0]
    i, y, x = (int(v) for v in wide)
    other = tuple(t.clone() for t in good)
    other[2][i, 0, y, x] = int(ref['prob'][i, :, y, x].topk(2)[1][1])
    assert rejected(other, ref, d, 'best moved where the gap is wide')


def test_compare_rejects_second_trip_pixels_under_the_first_samples_camera():
    """Defect (i), row 8 at 2 x 91 x 91: the pixels with ``pid >= 16384`` (all in sample 1) are computed under sample 0's camera
    ('forward' turns sample 1's view by 0.04 rad).  mv.compare accepts the float64 result itself and rejects the result with the defect
    on those 178 pixels alone."""
    for name in ('cap-2x91x91-d16', 'cap-2x91x91-d65'):
        (b, h, w), d, moves = mv.BOUNDARY[name]
        f0, f1, cam, cand, _ = mv.boundary_inputs(name)
        ref = mv.boundary_reference(name)
        good = mv.result_of(ref)
        assert not rejected(good, ref, d, f'{name} unmodified')
        assert not torch.equal(cam[:, 1], cam[:, 0])
        wrong = mv.result_of(mv.reference_of(f0[:, 1:], f1[:, 1:], h, w, cam[:, :1], cand))
        trip = mv.second_trip(b, h, w)
        bad = tuple(t.clone() for t in good)
        for t, e in zip(bad, wrong):
            t[1][:, trip[1]] = e[0][:, trip[1]]
        assert all(torch.equal(t[0], g[0]) and torch.equal(t[1][:, ~trip[1]], g[1][:, ~trip[1]]) for t, g in zip(bad, good))
        assert rejected(bad, ref, d, f'{name} second trip under the camera of sample 0')


def test_compare_rejects_a_source_count_clamped_at_three():
    """Defect (ii), row 9: ``sum_s v_sj l_sj`` divided by ``min(n_j, 3)`` -- what S <= 3 cannot tell from the rule."""
    for name in [n for n in mv.BOUNDARY if n.startswith(('s8-', 's5-'))]:
        (b, h, w), d, moves = mv.BOUNDARY[name]
        ref = mv.boundary_reference(name)
        assert not rejected(mv.result_of(ref), ref, d, f'{name} unmodified')
        total = ref['logits'] * ref['views'].clamp(min=1).double()
        cand = mv.candidates(d)
        bad = dict(ref, **mv.from_logits(total / ref['views'].clamp(1, 3).double(), cand, ref['stats'].in_view))
        assert rejected(mv.result_of(bad), ref, d, f'{name} n_j clamped at 3')
        # the same defect passes where no count exceeds 3: the cases the suite had
        small = mv.reference('B')
        kept = dict(small, **mv.from_logits(small['logits'] * small['views'].clamp(min=1).double() / small['views'].clamp(1, 3).double(),
                                            mv.candidates(mv.CASES['B'][1]), small['stats'].in_view))
        assert not rejected(mv.result_of(kept), small, mv.CASES['B'][1], 'case B n_j clamped at 3')


@pytest.mark.parametrize('case', ['B', 'C'])
def test_compare_rejects_a_row_of_segment_three_read_from_segment_two(case):
    """Defect (iii), row 10: the first row of segment 3 resolves to the same offset of segment 2 (a ``ptr3`` / ``first3`` that is never
    taken).  Segment 2's row is another operand, so the result is finite and plausible."""
    (b, h, w), d, moves = mv.CASES[case]
    cand = mv.candidates(d)
    segs, table, rows, use, ref = fu.edges_case(case)
    assert not rejected(mv.result_of(ref), ref, d, f'case {case} unmodified')
    swapped = [t.clone() for t in segs]
    swapped[3][0] = segs[2][0]
    assert bool(torch.isfinite(segs[2][0]).all()) and not torch.equal(segs[3][0], segs[2][0])
    g0, g1, gc, on = confidence.depth_rows_to_source_major_host(swapped, table, rows)
    bad = mv.reference_of(g0, g1, h, w, gc, cand, on)
    assert rejected(mv.result_of(bad), ref, d, f'case {case}: segment 3 row 0 read from segment 2')
