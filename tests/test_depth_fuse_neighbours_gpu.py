"""``um_depth_corr_softmax_multi_rows`` and ``forward_sequence(task='depth', fuse_neighbours=True)`` on the device.

The row-table launch is the contiguous fused launch (``um_depth_corr_softmax_multi``, gated against float64 in
tests/test_depth_multiview_gpu.py) with another operand addressing: every comparison of the two is bit for bit, on ``out``, ``stats``
and ``index``.  The model is compared with ``forward_multiview`` per frame (the oracle of the feature) and with the unfused sequence
under ``floor_close`` of tests/test_video_gpu.py (1e-3 x max(1, |want|max)): the same mathematics in another batch composition."""
import pytest
import torch

from tests import depth_fuse_neighbours_util as fu
from tests import depth_multiview_util as mv
from tests import memory_guard as mg
from tests.test_depth_sequence_gpu import _model, host_relative, scene
from tests.test_video_gpu import floor_close
from unimatch_amd import _abi, confidence
from unimatch_amd.ops import HipOps, KernelTimer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = ['A', 'B', 'C', 'D', 'one1']
SWEEPS = ('depth_corr_softmax', 'depth_corr_softmax_stats', 'depth_corr_softmax_multi', 'depth_corr_softmax_multi_rows')


@pytest.fixture(scope='module')
def ops():
    return HipOps('exact')


def dev(*tensors):
    return tuple(t.to(DEV) for t in tensors)


def by_rows(ops, segs, h, w, table, rows, cand, argmax=False, **kw):
    return ops.depth_corr_softmax(list(segs), None, h, w, table, cand, argmax, rows=rows, **kw)


def same(got, want, label):
    for name, a, e in zip(('out', 'stats', 'index'), got, want):
        assert a.dtype == e.dtype and torch.equal(a, e), (label, name, (a.double() - e.double()).abs().max().item())


# ------------------------------------------------------------------ 1. the rows launch is the contiguous launch, bit for bit
@pytest.mark.parametrize('argmax', [False, True])
@pytest.mark.parametrize('segments', [1, 2, 3, 4])
@pytest.mark.parametrize('case', CASES)
def test_rows_launch_is_the_contiguous_launch(ops, case, segments, argmax):
    (b, h, w), d, moves = mv.CASES[case]
    f0, f1, cam, cand = mv.inputs(case)
    segs, table, rows = fu.scatter(f0, f1, cam, segments, seed=len(case))
    want = ops.depth_corr_softmax(*dev(f0, f1), h, w, *dev(cam, cand), argmax, stats=True, peak_radius=2)
    got = by_rows(ops, dev(*segs), h, w, *dev(table, rows, cand), argmax, stats=True, peak_radius=2)
    assert tuple(got[0].shape) == (b, 1, h, w) and tuple(got[1].shape) == (b, 4, h, w) and tuple(got[2].shape) == (b, 2, h, w)
    same(got, want, (case, segments, argmax))
    assert torch.equal(by_rows(ops, dev(*segs), h, w, *dev(table, rows, cand), argmax), want[0])        # without the statistics


@pytest.mark.parametrize('d', [64, 80])
def test_the_table_of_a_sequence_chunk(ops, d):
    """The sequence's own pattern: tok0 | tok1 | the carried pair; the same row is f1 of one sample and f0 of the next one's second
    source, and a cam row serves one source only.  Against the contiguous launch on the gathered operands."""
    nb, h, w = 3, 9, 11
    f0, f1 = mv.features(nb, h, w, ('sideways', 'opposite'))
    tok0, tok1, carried = f0[0], f1[0], torch.stack([f1[1][0], f0[1][0]], 0)
    fwd, inv = mv.camera(nb + 1, h, w, 'sideways'), mv.camera(nb + 1, h, w, 'opposite')
    table = torch.cat([fwd, inv], 0)
    cand = mv.candidates(d)
    from unimatch_amd.model import neighbour_rows
    rows = neighbour_rows(nb, True)
    assert rows.dtype == torch.int32 and rows.tolist() == [[[0, 3, 1], [1, 4, 2], [2, 5, 3]], [[7, 6, 4], [3, 0, 5], [4, 1, 6]]]
    none = neighbour_rows(nb, False)
    assert none.tolist() == [[[0, 3, 0], [1, 4, 1], [2, 5, 2]], [[-1, -1, -1], [3, 0, 3], [4, 1, 4]]]
    g0, g1, gc, use = confidence.depth_rows_to_source_major_host([tok0, tok1, carried], table, rows)
    assert bool(use.all()) and torch.equal(g0[1, 1], tok1[0]) and torch.equal(g1[0, 0], tok1[0]) and torch.equal(g0[1, 0], carried[1])
    want = ops.depth_corr_softmax(*dev(g0.contiguous(), g1.contiguous()), h, w, *dev(gc.contiguous(), cand), stats=True)
    got = by_rows(ops, dev(tok0, tok1, carried), h, w, *dev(table, rows, cand), stats=True)
    same(got, want, 'carried')
    g0, g1, gc, use = confidence.depth_rows_to_source_major_host([tok0, tok1], table[[1, 2, 3, 5, 6, 7]], none)
    assert use.tolist() == [[True] * 3, [False, True, True]]
    want = ops.depth_corr_softmax(*dev(g0.contiguous(), g1.contiguous()), h, w, *dev(gc.contiguous(), cand), stats=True, use=use.to(DEV))
    got = by_rows(ops, dev(tok0, tok1), h, w, *dev(table[[1, 2, 3, 5, 6, 7]].contiguous(), none, cand), stats=True)
    same(got, want, 'first frame off')


# ------------------------------------------------------------------ 2. off rows
@pytest.mark.parametrize('case', ['A', 'B', 'C'])
def test_bad_indices_are_the_use_mask(ops, case):
    (b, h, w), d, moves = mv.CASES[case]
    f0, f1, cam, cand = mv.inputs(case)
    segs, table, rows = fu.scatter(f0, f1, cam, 3, seed=7)
    total = sum(t.shape[0] for t in segs)
    use = torch.ones(len(moves), b, dtype=torch.uint8)
    use[1, 0] = use[0, 1] = 0
    if len(moves) > 2:
        use[2, 1] = 0
    want = ops.depth_corr_softmax(*dev(f0, f1), h, w, *dev(cam, cand), stats=True, use=use.to(DEV))
    for shift in (0, 2, 4):                      # every kind of bad index, over the three rounds
        bad = fu.switch_off(rows, use, total, table.shape[0], shift)
        assert int((bad != rows).any(-1).sum()) == int((use == 0).sum())
        got = by_rows(ops, dev(*segs), h, w, *dev(table, bad, cand), stats=True)
        same(got, want, (case, shift))


@pytest.mark.parametrize('case', ['A', 'C', 'one1'])
def test_a_sample_with_every_source_off_is_exactly_uniform(ops, case):
    (b, h, w), d, moves = mv.CASES[case]
    f0, f1, cam, cand = mv.inputs(case)
    segs, table, rows = fu.scatter(f0, f1, cam, 2, seed=3)
    total = sum(t.shape[0] for t in segs)
    none = rows.clone()
    none[:, b - 1, 1] = torch.tensor([-1, total, fu.BIG][:len(moves)], dtype=torch.int32)
    use = torch.ones(len(moves), b, dtype=torch.uint8)
    use[:, b - 1] = 0
    want = ops.depth_corr_softmax(*dev(f0, f1), h, w, *dev(cam, cand), stats=True, use=use.to(DEV))
    got = by_rows(ops, dev(*segs), h, w, *dev(table, none, cand), stats=True)
    same(got, want, case)
    out, stats, index = (t.cpu() for t in got)
    assert bool((index[b - 1] == 0).all())                                          # best == 0 and in_view == 0
    assert bool((stats[b - 1, 0] == stats[b - 1, 0].flatten()[0]).all()) and abs(stats[b - 1, 0].flatten()[0].item() - 1.0 / d) <= 1e-7
    assert (out[b - 1].double() - cand.double().mean()).abs().max().item() <= mv.TOL * mv.scales(d)['out']


# ------------------------------------------------------------------ 3. memory contract
def test_memory_contract():
    """Red zones intact, placed inputs unchanged, results identical across the fills and across two runs.  The segments are allocated
    UNDER the guard (``torch.empty``: every row holds the run's fill byte) and only the rows the table names are written, so a row no
    entry names -- and every row of an off source, which is left at the fill -- changes from run to run: reading one would change the
    result.  After the launch every segment and the cam table hold the bytes they held before it."""

    def run(ops, g):
        res = []
        for case, segments, off, argmax in (('B', 3, False, False), ('C', 2, False, True), ('B', 1, True, False), ('C', 3, True, False)):
            (b, h, w), d, moves = mv.CASES[case]
            f0, f1, cam, cand = mv.inputs(case)
            segs, table, rows = fu.scatter(f0, f1, cam, segments, seed=11)
            use = torch.ones(len(moves), b, dtype=torch.bool)
            if off:
                use[1, 0] = use[0, 1] = False
                rows = fu.switch_off(rows, use, sum(t.shape[0] for t in segs), table.shape[0])
            named = [torch.zeros(t.shape[0], dtype=torch.bool) for t in segs]
            first = [0]
            for t in segs[:-1]:
                first.append(first[-1] + t.shape[0])
            cam_named = torch.zeros(table.shape[0], dtype=torch.bool)
            for s in range(len(moves)):
                for bb in range(b):
                    if use[s, bb]:
                        for r in rows[s, bb, :2].tolist():
                            i = max(n for n in range(len(segs)) if first[n] <= r)
                            named[i][r - first[i]] = True
                        cam_named[rows[s, bb, 2]] = True
            placed = []
            for t, keep in zip(segs, named):
                buf = torch.empty(tuple(t.shape), dtype=torch.float32, device=DEV)       # guarded: the run's fill in every row
                buf[keep.to(DEV)] = t[keep].to(DEV)
                placed.append(buf)
            cam_buf = torch.empty(tuple(table.shape), dtype=torch.float32, device=DEV)
            cam_buf[cam_named.to(DEV)] = table[cam_named].to(DEV)
            before = [t.view(torch.int32).clone() for t in placed + [cam_buf]]
            got = by_rows(ops, placed, h, w, cam_buf, g.place(rows), g.place(cand), argmax, stats=True, peak_radius=2)
            torch.cuda.synchronize()
            assert all(torch.equal(t.view(torch.int32), e) for t, e in zip(placed + [cam_buf], before))      # operands are read-only
            res += list(got)
        return res

    first = mg.contract(run, lambda guard: (guard,), device=DEV, make_ops=lambda: HipOps('exact'))
    assert first is not None
    assert any('ops.py' in site for site in mg.contract.last_sites)


@pytest.mark.parametrize('case', ['B', 'C'])
def test_stats_and_index_are_optional_in_the_abi(case):
    import ctypes
    (b, h, w), d, moves = mv.CASES[case]
    lib = _abi.load()
    f0, f1, cam, cand = mv.inputs(case)
    segs, table, rows = fu.scatter(f0, f1, cam, 2, seed=5)
    segs, (table, rows, cand) = dev(*segs), dev(table, rows, cand)
    ptrs = (ctypes.c_void_p * 2)(*[t.data_ptr() for t in segs])
    counts = (ctypes.c_int * 2)(*[t.shape[0] for t in segs])

    def call(with_stats, with_index):
        out = torch.full((b, 1, h, w), float('nan'), device=DEV)
        stats = torch.full((b, 4, h, w), -7.0, device=DEV)
        index = torch.full((b, 2, h, w), -7, dtype=torch.int32, device=DEV)
        _abi.check(lib.um_depth_corr_softmax_multi_rows(ptrs, counts, 2, table.data_ptr(), table.shape[0], rows.data_ptr(), cand.data_ptr(),
                                                        out.data_ptr(), stats.data_ptr() if with_stats else None,
                                                        index.data_ptr() if with_index else None, len(moves), b, h, w, mv.C, d, 0, 1,
                                                        torch.cuda.current_stream().cuda_stream), 'um_depth_corr_softmax_multi_rows')
        return out, stats, index

    out, stats, index = call(True, True)
    o1, s1, i1 = call(False, True)
    o2, s2, i2 = call(True, False)
    o3, s3, i3 = call(False, False)
    assert bool(torch.isfinite(out).all())
    assert torch.equal(o1, out) and torch.equal(o2, out) and torch.equal(o3, out)
    assert torch.equal(i1, index) and torch.equal(s2, stats)
    assert bool((s1 == -7).all()) and bool((i2 == -7).all()) and bool((s3 == -7).all()) and bool((i3 == -7).all())     # not written


def test_depth_match_multi_runs_the_rows_launch_on_cuda_tensors(ops):
    (b, h, w), d, moves = mv.CASES['A']
    f0, f1, cam, cand = mv.inputs('A')
    segs, table, rows = fu.scatter(f0, f1, cam, 3)
    ops.timer = timer = KernelTimer()
    out, st = confidence.depth_match_multi(list(dev(*segs)), None, h, w, *dev(table, cand), ops=ops, rows=rows.to(DEV))
    ops.timer = None
    assert [r[0] for r in timer.records] == ['depth_corr_softmax_multi_rows']
    want = ops.depth_corr_softmax(*dev(f0, f1), h, w, *dev(cam, cand), stats=True)
    assert torch.equal(out, want[0]) and torch.equal(st.max_prob, want[1][:, 0]) and torch.equal(st.in_view, want[2][:, 1])
    with pytest.raises(ValueError, match='rows'):
        ops.depth_corr_softmax(list(dev(*segs)), None, h, w, table.to(DEV), cand.to(DEV), rows=rows.to(DEV).long())
    with pytest.raises(ValueError, match='segment 1'):
        ops.depth_corr_softmax([segs[0].to(DEV), segs[1]], None, h, w, table.to(DEV), cand.to(DEV), rows=rows.to(DEV))


# ------------------------------------------------------------------ 4. the model
@pytest.mark.parametrize('name', ['gmdepth_s1', 'gmdepth_s1_rr1'])
def test_fused_sequence(name):
    model, kw = _model(name)
    model.launch_parts = 1
    T, H, W = 6, 96, 128
    x, k, poses = scene(T, H, W, seed=177)
    rel = host_relative(poses).to(DEV)
    poses = poses.to(DEV)
    args = dict(task='depth', intrinsics=k, pairs_per_launch=3, **kw)
    model.ops.timer = timer = KernelTimer()
    plain = model.forward_sequence(x, poses=poses, return_confidence=True, **args)
    model.ops.timer = None
    plain_names = [r[0] for r in timer.records]
    calls = [0]
    inner = model.backbone.forward

    def counted(x, *a, **kws):
        calls[0] += (x.shape[0] if torch.is_tensor(x) else sum(t.shape[0] for t in x))
        return inner(x, *a, **kws)
    model.backbone.forward = counted
    model.ops.timer = timer = KernelTimer()
    try:
        out = model.forward_sequence(x, poses=poses, fuse_neighbours=True, return_confidence=True, **args)
    finally:
        del model.backbone.forward
        model.ops.timer = None
    names = [r[0] for r in timer.records]
    assert calls[0] == T                                                                  # the encoder sees T images
    assert set(out) == {'depth', 'depth_confidence', 'carry'} and tuple(out['depth'].shape) == (T - 1, H, W)
    assert bool(torch.isfinite(out['depth']).all())
    # one rows launch per chunk (3 + 2 pairs) and no other plane sweep; the Transformer's work is the unfused call's
    assert [n for n in names if n in SWEEPS] == ['depth_corr_softmax_multi_rows'] * 2
    assert [n for n in plain_names if n in SWEEPS] == ['depth_corr_softmax_stats'] * 2
    attn = lambda ns: [n for n in ns if 'attn' in n]
    assert attn(names) == attn(plain_names) and len(attn(names)) > 0
    assert [n for n in names if n not in SWEEPS] == [n for n in plain_names if n not in SWEEPS]       # ... and so is everything else
    # every interior frame against forward_multiview, frame 0 against the unfused sequence
    for t in range(1, T - 1):
        srcs = torch.stack([x[t + 1], x[t - 1]], 0)[None].contiguous()
        pose = torch.stack([rel[t], torch.linalg.inv(rel[t - 1].cpu()).to(DEV)], 0)[None].contiguous()
        want = model.forward_multiview(x[t:t + 1], srcs, intrinsics=k, poses=pose, **kw)['flow_preds'][0][0]
        floor = 1e-3 * max(1.0, want.abs().max().item())
        print(f'{name} frame {t}: |fused - multiview| {(out["depth"][t] - want).abs().max().item():.3e}, '
              f'|unfused - multiview| {(plain["depth"][t] - want).abs().max().item():.3e}, floor {floor:.3e}')
        assert floor_close(out['depth'][t], want), t
    print(f'{name} frame 0: |fused - unfused| {(out["depth"][0] - plain["depth"][0]).abs().max().item():.3e}')
    assert floor_close(out['depth'][0], plain['depth'][0])
    # the union of two views sees at least what one sees: source 0's coordinates are computed identically
    seen, one = out['depth_confidence']['in_view'], plain['depth_confidence']['in_view']
    assert tuple(seen.shape) == (T - 1, H // 8, W // 8) and bool((seen >= one).all()) and torch.equal(seen[0], one[0])
    # repeated, without the statistics, and fed in pieces with the carry: [:4] is 3 pairs, [4:] behind the carry 2 -- the chunk shapes
    again = model.forward_sequence(x, poses=poses, fuse_neighbours=True, **args)
    assert set(again) == {'depth', 'carry'} and torch.equal(again['depth'], out['depth'])
    a = model.forward_sequence(x[:4], poses=poses[:4], fuse_neighbours=True, return_confidence=True, **args)
    b = model.forward_sequence(x[4:], poses=poses[4:], fuse_neighbours=True, return_confidence=True, carry=a['carry'], **args)
    assert torch.equal(torch.cat([a['depth'], b['depth']], 0), out['depth'])
    for key in ('max_prob', 'best', 'in_view'):
        assert torch.equal(torch.cat([a['depth_confidence'][key], b['depth_confidence'][key]], 0), out['depth_confidence'][key]), key
    # without the keyword nothing changes
    off = model.forward_sequence(x, poses=poses, fuse_neighbours=False, return_confidence=True, **args)
    assert torch.equal(off['depth'], plain['depth']) and set(off['carry']) == set(plain['carry'])
    model.check_operand_range()


def test_fused_sequence_never_synchronises():
    model, kw = _model('gmdepth_s1_rr1')
    x, k, poses = scene(5, 96, 128, seed=178)
    poses = poses.to(DEV)
    args = dict(task='depth', intrinsics=k, poses=poses, pairs_per_launch=2, fuse_neighbours=True, colorize=True, return_confidence=True,
                **kw)
    first = model.forward_sequence(x, **args)                           # library, allocator, weight planes, tables warm
    head = model.forward_sequence(x[:3], **dict(args, poses=poses[:3]))
    model.forward_sequence(x[3:], **dict(args, poses=poses[3:], carry=head['carry']))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=DEV).item()                             # the mode does catch a synchronising call
        got = model.forward_sequence(x, **args)
        head = model.forward_sequence(x[:3], **dict(args, poses=poses[:3]))
        piece = model.forward_sequence(x[3:], **dict(args, poses=poses[3:], carry=head['carry']))
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    for key in ('depth', 'depth_rgb'):
        assert torch.equal(got[key], first[key]), key
        assert torch.equal(piece[key], first[key][2:]), key
