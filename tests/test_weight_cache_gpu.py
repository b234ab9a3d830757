"""Cached weight planes must follow every change of the weights (tests/weight_cache_util.py has the why).

Everywhere the trusted evaluation is the same model after ``invalidate_weights()``, which clears every cache entry and rebuilds from
the parameters; per setup it is anchored once, bitwise, against a newly built model with its own new ``HipOps`` that loaded the final
``state_dict``.  All images are ``synth_images(B, 64, 128, seed=5, kind='shift')``.
"""
import functools
import gc
import time
import weakref

import pytest
import torch

from oracle import hotpath as hp
from tests.weight_cache_util import CACHE_TAGS, NO_EFFECT, PARAMETER_COUNTS, SETUPS, cache_kinds, perturb_, tag_kind
from unimatch_amd import UniMatch
from unimatch_amd.ops import HipOps
from unimatch_amd.synth import CONFIGS, synth_camera, synth_images, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEEN = {}                                # setup -> kinds of cache entry its forward built (filled by sections 1 and 2)


def rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@functools.lru_cache(maxsize=None)
def _state(config, seed=326):
    ck, _ = CONFIGS[config]
    shapes = {k: v.shape for k, v in UniMatch(**ck).state_dict().items()}
    return synth_state_dict(shapes, seed=seed, **({'refine_gain': 0.02} if ck['reg_refine'] else {}))


@functools.lru_cache(maxsize=None)
def _inputs(config, batch):
    _, fk = CONFIGS[config]
    i0, i1 = synth_images(batch, 64, 128, seed=5, kind='shift', normalized=(fk['task'] != 'flow'))
    kw = dict(fk)
    if fk['task'] == 'depth':
        k, pose = synth_camera(batch, 64, 128)
        kw.update(intrinsics=k.to(DEV), pose=pose.to(DEV))
    return i0.to(DEV), i1.to(DEV), kw


def _flags(model, setup):
    for k, v in SETUPS[setup][1].items():                          # attributes of the HipOps instance
        setattr(model.ops, k, v)


def build(setup, state=None, precision='exact'):
    config = SETUPS[setup][0]
    model = UniMatch(**CONFIGS[config][0]).eval()
    model.load_state_dict(state if state is not None else _state(config))
    model = model.to(DEV)
    if precision != 'exact':
        model.set_precision(precision)
    _flags(model, setup)
    return model


def run(model, setup, batch=1, call=None):
    """Every prediction of one forward, flattened into one tensor."""
    i0, i1, kw = _inputs(SETUPS[setup][0], batch)
    preds = (call or model)(i0, i1, **kw)['flow_preds']
    return torch.cat([p.reshape(-1) for p in preds]).clone()


def trusted(model, setup, batch=1):
    model.invalidate_weights()
    return run(model, setup, batch)


def anchored(model, setup, want, precision='exact'):
    """``want`` (this model's trusted result) is bitwise what a new model with a new backend computes from the same state_dict."""
    fresh = build(setup, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, precision)
    assert fresh.ops is not model.ops
    assert torch.equal(run(fresh, setup), want), f'{setup}: invalidate_weights() does not give what a new model gives'
    return fresh


# ------------------------------------------------------------------------------------------------ 1. per-parameter sweep
@pytest.mark.parametrize('setup', list(SETUPS))
def test_every_parameter_reaches_the_next_forward(setup):
    """After a warm forward every parameter is edited in turn (in place, cumulative); the next forward -- which finds every cache
    entry of the forward before in place -- must be bitwise the forward after ``invalidate_weights()``, and that one must differ
    from the one before the edit unless the parameter is listed with a reason in NO_EFFECT."""
    config, _, prefix = SETUPS[setup]
    t0 = time.perf_counter()
    model = build(setup)
    ops = model.ops
    warm = run(model, setup)
    SEEN[setup] = cache_kinds(ops)
    previous = trusted(model, setup)
    assert torch.equal(warm, previous) and torch.isfinite(warm).all()
    g = torch.Generator().manual_seed(20240611)
    exempt = NO_EFFECT[config] if not prefix else {}
    stale, unchanged, swept = [], [], 0
    for name, p in model.named_parameters():
        if not name.startswith(prefix):
            continue
        swept += 1
        perturb_(p, g)
        cached = run(model, setup)
        fresh = trusted(model, setup)
        if not torch.equal(cached, fresh):
            stale.append(name)
        if torch.equal(fresh, previous) != (name in exempt):
            unchanged.append(name)
        previous = fresh
    torch.cuda.synchronize()
    took = time.perf_counter() - t0
    print(f'{setup}: {swept} parameters swept in {took:.2f} s, {len(ops._wcache)} cache entries, kinds {sorted(SEEN[setup])}')
    assert swept == (PARAMETER_COUNTS[config] if not prefix else 96), swept     # 6 blocks x (6 + 10) Transformer parameters
    assert not stale, f'{setup}: the forward after an edit of these parameters used planes of the old weights: {stale}'
    assert not unchanged, (f'{setup}: the trusted forward did not change with these parameters (or changed with an exempt one): '
                           f'{unchanged}')
    assert torch.isfinite(previous).all()
    assert ops is model.ops and len(ops._wcache) <= 257            # the bound the prune keeps
    assert SEEN[setup] <= CACHE_TAGS
    anchored(model, setup, previous)


# ------------------------------------------------------------------------------------------------ 2. kinds of change
# one parameter per kind of cache entry: (setup, kind, position of the parameter among the entry's key tensors)
REPRESENTATIVES = [
    ('gmflow_s2_rr6', 'stem', 0), ('gmflow_s2_rr6', 'conv', 0), ('gmflow_s2_rr6', 'lin', 0),
    ('gmflow_s2_rr6', 'fold_q', 0),                                # k_proj.weight: only the folded query weight reads it
    ('gmflow_s2_rr6', 'fold_m', 1),                                # v_proj.weight: only the folded merge weight reads it
    ('gmflow_s2_rr6', 'conv7', 0),
    ('gmflow_s2_rr6', ('refine', 'mo'), 1),                        # a bias the entry holds a zero-padded copy of
    ('gmflow_s2_rr6', ('refine', 'zr1v'), 2),                      # r's weight in the hoisted gate convolution
    ('gmflow_s1', 'padw', 0),                                      # the upsampler's first convolution, zero-padded input channels
    ('gmflow_s1-unfolded', 'kv4', 2), ('gmflow_s1-unfolded', 'lin', 0),
]


def _representative(model, kind, position):
    """The first cache entry of this kind whose key tensor at ``position`` is a parameter -> its name.  ('lin' and 'conv' entries
    keyed by a folded or padded tensor map to no parameter and are passed over: the parameter they were built from is the
    representative of 'fold_*' and 'padw'.)"""
    names = {id(p): n for n, p in model.named_parameters()}
    for key in model.ops._wcache:
        if kind in (key[0], tag_kind(key[0])) and len(key) > 1 + position and key[1 + position][0] in names:
            return names[key[1 + position][0]]
    raise AssertionError(f'no {kind!r} entry keyed by a parameter among {sorted(cache_kinds(model.ops))}')


@pytest.mark.parametrize('setup,kind,position', REPRESENTATIVES, ids=[f'{s}-{"_".join(k) if isinstance(k, tuple) else k}' for s, k, _ in REPRESENTATIVES])
def test_every_kind_of_change_reaches_the_next_forward(setup, kind, position):
    model = build(setup)
    first = run(model, setup)
    SEEN.setdefault(setup, set()).update(cache_kinds(model.ops))
    name = _representative(model, kind, position)
    param = dict(model.named_parameters())[name]
    state = {'before': first}

    def settle(label, got):
        want = trusted(model, setup)
        assert torch.equal(got, want), f'{name} ({kind}), {label}: the forward used planes of the old weights'
        assert not torch.equal(want, state['before']), f'{name} ({kind}), {label}: the change did not reach the trusted forward'
        state['before'] = want

    with torch.no_grad():                                           # (a) in place, the version moves
        param.mul_(1.1)
    settle('in place under no_grad', run(model, setup))

    param.data = param.data.clone() * 1.1                           # (b) new storage, same version
    settle('p.data = new tensor', run(model, setup))

    param.data.mul_(1.1)                                            # (c) invisible edit + invalidate_weights()
    model.invalidate_weights()
    settle('.data edit + invalidate_weights()', run(model, setup))

    model.check_weights = True                                      # (d) invisible edit under the per-forward fingerprint
    param.data.mul_(1.1)
    settle('.data edit with check_weights', run(model, setup))
    param.data.mul_(1.1)                                            # ... and once more, now against a stored fingerprint
    settle('second .data edit with check_weights', run(model, setup))
    model.check_weights = False

    changed = {k: v.detach().clone() for k, v in model.state_dict().items()}        # (e) load_state_dict
    changed[name] *= 1.1
    model.load_state_dict(changed)
    settle('load_state_dict', run(model, setup))

    model.cpu()                                                     # (f) a round trip through the CPU with an edit there
    dict(model.named_parameters())[name].data.mul_(1.1)
    model.to(DEV)
    assert model.ops is not None
    settle('cpu(), edit, to(cuda)', run(model, setup))
    anchored(model, setup, state['before'])


@pytest.mark.parametrize('setup', ['gmflow_s2_rr6', 'gmflow_s1', 'gmflow_s1-unfolded'])
def test_set_precision_rebuilds_every_plane(setup):
    """(g) 'fast' after warm 'exact' forwards is bitwise a new fast model, and back in 'exact' the first result returns."""
    model = build(setup)
    exact = run(model, setup)
    old = model.ops
    model.set_precision('fast')
    _flags(model, setup)
    assert model.ops is not old
    fast = run(model, setup)
    assert torch.isfinite(fast).all() and not torch.equal(fast, exact)
    anchored(model, setup, fast, precision='fast')
    model.set_precision('exact')
    _flags(model, setup)
    assert torch.equal(run(model, setup), exact)


def test_the_sweeps_reach_every_kind_of_cache_entry():
    """The union of the kinds of entry that the setups of sections 1 and 2 build is CACHE_TAGS -- the set
    tests/test_weight_cache_cpu.py ties to the ``_cache_get`` call sites.  (A setup whose test did not run in this session is
    run here.)"""
    for setup in SETUPS:
        if setup not in SEEN:
            model = build(setup)
            run(model, setup)
            SEEN[setup] = cache_kinds(model.ops)
    union = set().union(*SEEN.values())
    assert union == set(CACHE_TAGS), {s: sorted(k) for s, k in SEEN.items()}
    assert 'kv4' not in SEEN['gmflow_s1'] and 'kv4' in SEEN['gmflow_s1-unfolded'] and 'kv4' in SEEN['gmflow_s1-unfolded-fused_kv']
    assert 'padw' in SEEN['gmflow_s1'] and 'refine' in SEEN['gmdepth_s1_rr1']


# ------------------------------------------------------------------------------------------------ 4. backend-level cases
def _planes(ops, w):
    return (ops.weight_planes((w,)) if w.dim() == 2 else ops.conv_weight_planes(w))[0]


def _at_address(address, make, what):
    """A new tensor at ``address`` (the caching allocator hands a freed block to the next request of its size).  That reuse is the
    premise of the caller's test: without it the test fails -- it is never skipped silently."""
    kept = []
    for attempt in range(8):
        t = make(attempt)
        if t.data_ptr() == address:
            return t
        kept.append(t)                                              # stays allocated: the next request gets another block
    pytest.fail(f'premise not met: none of 8 new allocations landed on the freed address of {what}')


@pytest.mark.parametrize('shape', [(128, 128), (64, 64, 3, 3)])
def test_a_new_weight_at_a_freed_address_gets_its_own_planes(shape):
    ops = HipOps('exact')
    w = rnd(1, *shape, scale=0.05).to(DEV)
    old = _planes(ops, w).clone()
    address, version = w.data_ptr(), w._version
    del w
    w2 = _at_address(address, lambda i: rnd(2 + i, *shape, scale=0.05).to(DEV), 'the first weight')
    assert w2._version == version                                   # same address, version, shape, dtype: only the object differs
    got = _planes(ops, w2)
    assert torch.equal(got, _planes(HipOps('exact'), w2)) and not torch.equal(got, old)
    if len(shape) == 2:
        # a folded pair: its planes are keyed by the folded tensor, which only the 'fold_q' entry keeps alive
        a, b = rnd(20, 128, 128, scale=0.05).to(DEV), rnd(21, 128, 128, scale=0.05).to(DEV)
        old = ops.weight_planes((ops._folded_weight('q', a, b),))[0].clone()
        address = a.data_ptr()
        del a
        a2 = _at_address(address, lambda i: rnd(30 + i, 128, 128, scale=0.05).to(DEV), 'the first factor of the fold')
        got = ops.weight_planes((ops._folded_weight('q', a2, b),))[0]
        new = HipOps('exact')
        assert torch.equal(got, new.weight_planes((new._folded_weight('q', a2, b),))[0]) and not torch.equal(got, old)


def test_the_cache_overflows_without_serving_a_wrong_entry():
    """300 distinct LIVE weights (Linear and convolution alternating) go through one backend: the prune finds nothing dead and
    drops everything.  A folded pair sits on either side of it: the first pair's fold and planes are the 256th and 257th
    insertion, the second pair's fold is the insertion that prunes."""
    ops, new = HipOps('exact'), HipOps('exact')
    weights = [rnd(100 + i, *((128, 128) if i % 2 == 0 else (64, 64, 3, 3)), scale=0.05).to(DEV) for i in range(300)]
    pairs = [tuple(rnd(500 + 2 * j + i, 128, 128, scale=0.05).to(DEV) for i in range(2)) for j in range(2)]
    held, folded = [], []
    for i, w in enumerate(weights):
        if i == 255:
            assert len(ops._wcache) == 255
            for a, b in pairs:
                f = ops._folded_weight('m', a, b)
                folded.append((f, ops.weight_planes((f,))[0]))
            assert len(ops._wcache) <= 257                          # 257 entries, then the prune (today it drops everything)
        held.append(_planes(ops, w))
        assert len(ops._wcache) <= 257
    for w, had in list(zip(weights, held))[:1] + list(zip(weights, held))[254:258]:
        assert torch.equal(_planes(ops, w), _planes(new, w)) and torch.equal(had, _planes(new, w))
    for (a, b), (f, had) in zip(pairs, folded):
        f_now, f_new = ops._folded_weight('m', a, b), new._folded_weight('m', a, b)
        assert torch.equal(f_now, f_new) and torch.equal(f, f_new)
        assert torch.equal(ops.weight_planes((f_now,))[0], new.weight_planes((f_new,))[0])
        assert torch.equal(had, new.weight_planes((f_new,))[0])
    # the kernel on the first weight's planes, as test_linear_planes_and_gelu checks it
    a = rnd(70, 300, 128, scale=2.0)
    want = a.double() @ weights[0].double().cpu().t()
    got, m, n = ops.linear_planes(a.to(DEV), (weights[0],))
    got = got.cpu().view(torch.float16).view(2, m, n).float().sum(0)
    assert (got.double() - want).abs().max().item() < 2e-5 * max(1.0, want.abs().max().item())


def test_two_models_share_one_backend():
    ops = HipOps('exact')
    models = [build('gmflow_s1', _state('gmflow_s1', seed)).bind_ops(ops) for seed in (326, 327)]
    first = [run(m, 'gmflow_s1') for m in models]
    assert not torch.equal(first[0], first[1])
    for _ in range(3):
        for m, want in zip(models, first):
            assert m.ops is ops and torch.equal(run(m, 'gmflow_s1'), want)
    anchored(models[1], 'gmflow_s1', first[1])


def test_cost_volume_feature_planes_follow_their_tokens():
    """``HipOps._k4_feat``: the operand planes of the cost volume's two token tensors, kept for the refinement loop's next
    iteration.  A hit (the same objects), ``f0.copy_(new)`` (the version moves) and new tensors at the freed addresses (only the
    objects differ), each against the fp64 oracle at the mean-error bound of test_cost_volume_matrix_core_path.

    Audit of tensors written by pointer (a kernel write through ``data_ptr`` moves no ``_version``, so such a tensor must never be
    a cache key).  ``HipOps`` methods that write into a tensor the caller supplies: ``convex_upsample(out=)``,
    ``image_prepare(out=)``, ``pred_restore(out=)``, ``conv_ex(out=, outp=)``, ``conv_gru(hidden, outp, z_out=, hidden_out=)``,
    ``conv7(out=, outp=)``, ``nhwc_gate(dest)``, ``local_corr_with_flow_planes(dest)``.  What model.py, encoder.py, refine.py and
    refine_nhwc.py pass there: the prediction tensor of a batch run in parts (``pred_out``), the prepared images / restored
    predictions of ``predict``, the upsampler's hidden planes, and the refinement block's own ``proj``, ``P[*]``, ``H``, ``ZR``,
    ``D``, ``mask`` and plane buffers ``G``, ``C1``, ``CF``, ``FH``, ``F1``, ``CORR``.  None of them is ever passed to
    ``_cache_get`` (whose keys are parameters, folded and padded weights only) or to ``_k4_feat_planes`` (whose keys are the
    per-forward views ``ori0`` / ``ori1`` of the encoder's output -- new tensors, hence new objects, in every forward; a stale
    object fails the weak-reference check, which the last step here exercises).  No such key exists, so there is nothing to fix."""
    ops = HipOps('exact')
    b, h, w = 1, 16, 32
    tok = lambda f: f.flatten(2).transpose(1, 2).contiguous()
    maps = [(rnd(40 + 2 * i, b, 128, h, w), rnd(41 + 2 * i, b, 128, h, w)) for i in range(3)]
    flow = rnd(50, b, 2, h, w, scale=2.5).contiguous()

    def check(t0, t1, f0, f1, label):
        want = hp.local_corr_with_flow(f0.double(), f1.double(), flow.double(), 4)
        got = ops.local_corr_with_flow(t0, t1, flow.to(DEV), h, w, 4)
        mean = (got.double().cpu() - want).abs().mean().item()
        assert mean < 3e-6 * max(1.0, want.abs().max().item()), (label, mean)
        return got

    t0, t1 = tok(maps[0][0]).to(DEV), tok(maps[0][1]).to(DEV)
    assert ops._k4_feat_planes(t0, t1, h, w, 4) is not None         # the matrix-core kernel with its cached planes serves this geometry
    first = check(t0, t1, *maps[0], 'first')
    planes = ops._k4_feat[3]
    assert torch.equal(check(t0, t1, *maps[0], 'hit'), first) and ops._k4_feat[3] is planes
    t0.copy_(tok(maps[1][0]))
    check(t0, t1, maps[1][0], maps[0][1], 'f0.copy_(new)')
    assert ops._k4_feat[3] is not planes
    a0, a1 = t0.data_ptr(), t1.data_ptr()
    del t0
    t0 = _at_address(a0, lambda i: tok(maps[2][0]).to(DEV), 'f0')
    del t1
    t1 = _at_address(a1, lambda i: tok(maps[2][1]).to(DEV), 'f1')
    check(t0, t1, *maps[2], 'new tensors at the old addresses')


# ------------------------------------------------------------------------------------------------ 5. concurrent parts and graph
def test_concurrent_parts_see_an_edit():
    """Batch 2 as two parts.  After an in-place edit the first forward runs the parts one after the other (it rebuilds shared cache
    entries), the second on two streams; both are the trusted result of one part."""
    setup = 'gmflow_s1'
    model = build(setup)
    model.launch_parts = 2
    a, b = run(model, setup, 2), run(model, setup, 2)               # sequential, then concurrent
    assert torch.equal(a, b)
    perturb_(model.transformer.layers[3].cross_attn_ffn.q_proj.weight, torch.Generator().manual_seed(9))
    with torch.no_grad():
        model.backbone.conv2.bias.add_(0.01)
    first, second = run(model, setup, 2), run(model, setup, 2)
    third = run(model, setup, 2)
    torch.cuda.synchronize()
    model.launch_parts = 1
    want = trusted(model, setup, 2)
    print('parts=2 after the edit: max |first - whole-batch trusted| =', (first - want).abs().max().item())
    assert not torch.equal(want, a)
    assert torch.equal(first, want) and torch.equal(second, want) and torch.equal(third, want)


def test_graph_replay_follows_the_weights():
    """A captured graph holds the addresses of the weight planes of its capture, while biases are read in place: after a change of
    the weights a replay would mix new biases with old planes.  The weights' state is part of what a graph is valid for: each
    replay is bitwise the eager forward of the current weights, one capture per weight state, superseded graphs are released."""
    from unimatch_amd.graph import GraphedUniMatch
    setup = 'gmflow_s1'
    model = build(setup)
    graphed = GraphedUniMatch(model)
    captures = []
    plain_capture = graphed._capture
    graphed._capture = lambda *a, **k: (captures.append(1), plain_capture(*a, **k))[1]
    eager = lambda: run(model, setup, 2)
    replay = lambda: run(model, setup, 2, call=graphed)
    first = replay()
    assert torch.equal(first, eager()) and torch.equal(replay(), first) and len(captures) == 1
    entry = next(iter(graphed._graphs.values()))
    dead = [weakref.ref(entry['out'])] + [weakref.ref(t) for t in entry['workspaces'].values()]
    del entry

    perturb_(model.transformer.layers[2].self_attn.merge.weight, torch.Generator().manual_seed(3))     # (a), replay first
    with torch.no_grad():
        model.upsampler[0].weight.mul_(1.05)
        model.upsampler[0].bias.add_(0.01)
    got = replay()
    want = eager()
    assert not torch.equal(want, first)
    assert torch.equal(got, want), 'replay after an in-place edit: not the eager forward of the current weights'
    assert torch.equal(replay(), want) and len(captures) == 2
    gc.collect()
    assert all(r() is None for r in dead), 'the superseded graph still holds its output or workspaces'

    model.load_state_dict(_state('gmflow_s1', seed=327))            # (e), eager first
    want = eager()
    assert torch.equal(replay(), want) and torch.equal(replay(), want) and len(captures) == 3

    i0, i1 = synth_images(2, 64, 128, seed=6, kind='shift')          # new inputs: the same graph
    i0, i1 = i0.to(DEV), i1.to(DEV)
    kw = _inputs('gmflow_s1', 2)[2]
    for _ in range(2):
        assert torch.equal(graphed(i0, i1, **kw)['flow_preds'][0], model(i0, i1, **kw)['flow_preds'][0])
    assert len(captures) == 3 and len(graphed._graphs) == 1 and all(v is not False for v in graphed._graphs.values())
