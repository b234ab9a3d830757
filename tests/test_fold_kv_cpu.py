"""k_proj / v_proj folded into the query and merge weights (``HipOps.fold_kv``): what can be checked without a GPU.

The identity.  A TransformerLayer of the reference is single-head, every Linear is bias-free and nothing non-linear sits between the
projections and the attention (unimatch/transformer.py:23-27, 58-60, 137), so with ``x`` the query stream and ``y`` the key / value stream

    (x Wq^T)(y Wk^T)^T = (x (Wk^T Wq)^T) y^T            merge(P (y Wv^T)) = (P y)(Wm Wv)^T

and the layer with ``q_proj' = Wk^T Wq``, ``merge' = Wm Wv``, ``k_proj = v_proj = I`` is the same function.  The fp64 oracle
(oracle/hotpath.py) evaluates both forms; they may differ by fp64 round-off only.

Bound of the identity test: outputs are O(1) (a LayerNorm's output plus the residual).  One fp64 operation carries 1.1e-16; a
projection sums 128 products (~3e-14 relative to the operands) and twelve attention layers with their softmaxes amplify that by a few
orders of magnitude at most.  1e-9 leaves five orders of magnitude above a single summation's error and stays 60 times below ONE
fp32 rounding of an O(1) value (6e-8): a fold that is wrong in any term, or formed in fp32, cannot pass.

The cache.  Folded weights are cached by ``HipOps._folded_weight`` next to the weight planes (same key: identity + version of the
parameters; same invalidation: ``invalidate_weights``), and their planes by ``weight_planes`` keyed by the folded tensor.  The kernels
need a GPU; the bookkeeping does not: ``weight_planes`` is replaced by a recorder here.
"""
import pytest
import torch

from oracle import hotpath as hp
from unimatch_amd import UniMatch
from unimatch_amd.model import FeatureTransformer
from unimatch_amd.ops import HipOps, fold_weights
from unimatch_amd.synth import synth_state_dict

IDENTITY_BOUND = 1e-9


def _weights(seed=7):
    proto = FeatureTransformer()
    return synth_state_dict({k: v.shape for k, v in proto.state_dict().items()}, seed=seed)


def folded_state_dict(sd):
    """The state dict of the folded model: q_proj' = Wk^T Wq, merge' = Wm Wv (``fold_weights``: fp64, rounded once to fp32),
    k_proj = v_proj = I."""
    out = dict(sd)
    eye = torch.eye(128)
    for name in sd:
        if name.endswith('q_proj.weight'):
            p = name[:-len('q_proj.weight')]
            out[p + 'q_proj.weight'] = fold_weights('q', sd[p + 'k_proj.weight'], sd[p + 'q_proj.weight'])
            out[p + 'merge.weight'] = fold_weights('m', sd[p + 'merge.weight'], sd[p + 'v_proj.weight'])
            out[p + 'k_proj.weight'] = out[p + 'v_proj.weight'] = eye
    return out


def test_fold_weights_is_the_fp64_product_rounded_once():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(128, 128, generator=g) * 0.1, torch.randn(128, 128, generator=g) * 0.1
    q, m = fold_weights('q', a, b), fold_weights('m', a, b)
    assert q.dtype == m.dtype == torch.float32 and q.is_contiguous() and m.is_contiguous()
    # one rounding to fp32 of the exact product: half an fp32 ulp of the entry (entries are below 0.5 here: ulp <= 2^-25)
    assert (q.double() - a.double().t() @ b.double()).abs().max() <= 2.0 ** -25 * 0.5 + 1e-15
    assert (m.double() - a.double() @ b.double()).abs().max() <= 2.0 ** -25 * 0.5 + 1e-15
    with pytest.raises(ValueError):
        fold_weights('k', a, b)


@pytest.mark.parametrize('h,w', [(24, 40), (32, 48)])
@pytest.mark.parametrize('attn_type,splits', [('swin', 2), ('self_swin2d_cross_1d', 2)])
def test_folded_transformer_is_the_unfolded_one_in_fp64(h, w, attn_type, splits):
    """Six blocks (odd ones shifted), 2-D swin self attention with K = 2 and either 2-D swin or whole-scanline 1-D cross attention.
    The folded weights are formed in fp64 here (not rounded to fp32): this is the algebra, not the rounding."""
    sd = {k: v.double() for k, v in _weights().items()}
    fd = dict(sd)
    eye = torch.eye(128, dtype=torch.float64)
    for name in sd:
        if name.endswith('q_proj.weight'):
            p = name[:-len('q_proj.weight')]
            fd[p + 'q_proj.weight'] = sd[p + 'k_proj.weight'].t() @ sd[p + 'q_proj.weight']
            fd[p + 'merge.weight'] = sd[p + 'merge.weight'] @ sd[p + 'v_proj.weight']
            fd[p + 'k_proj.weight'] = fd[p + 'v_proj.weight'] = eye
    g = torch.Generator().manual_seed(11)
    f0, f1 = torch.randn(1, 128, h, w, generator=g).double(), torch.randn(1, 128, h, w, generator=g).double()
    want = hp.feature_transformer(f0, f1, sd, attn_type, splits)
    got = hp.feature_transformer(f0, f1, fd, attn_type, splits)
    for a, b in zip(got, want):
        worst = (a - b).abs().max().item()
        print(f'{attn_type} {h}x{w}: folded vs unfolded fp64, max |diff| = {worst:.3e} (|out| max {b.abs().max().item():.2f})')
        assert worst < IDENTITY_BOUND, worst


def test_fold_weights_rounded_to_fp32_stay_inside_the_fp32_noise():
    """``fold_weights`` as the product uses it (rounded once to fp32) in the fp64 oracle: the distance to the unfolded fp64 model is that
    of ONE fp32 rounding of the weights -- below the distance of the fp32 evaluation of the unfolded model itself."""
    sd = _weights()
    g = torch.Generator().manual_seed(12)
    f0, f1 = torch.randn(1, 128, 24, 40, generator=g), torch.randn(1, 128, 24, 40, generator=g)
    d = lambda s, dt: hp.feature_transformer(f0.to(dt), f1.to(dt), {k: v.to(dt) for k, v in s.items()}, 'swin', 2)
    want, port, fold = d(sd, torch.float64), d(sd, torch.float32), d(folded_state_dict(sd), torch.float64)
    e_port = max((a.double() - b).abs().mean().item() for a, b in zip(port, want))
    e_fold = max((a - b).abs().mean().item() for a, b in zip(fold, want))
    print(f'mean |err| vs fp64: fp32 port {e_port:.3e}, fp64 with fp32-rounded folded weights {e_fold:.3e}')
    assert e_fold < e_port


# ------------------------------------------------------------------------------------------------ the cache
class _Recorder(HipOps):
    """HipOps without a GPU: the cache bookkeeping is the real one, ``weight_planes`` records what it is asked to build."""

    def __init__(self):                                            # (HipOps.__init__ loads the library and needs a device)
        self._wcache, self._entries, self.cache_generation = {}, {}, 0
        self.built = []

    def weight_planes(self, weights):
        key, hit = self._cache_get('lin', weights)
        if hit is not None:
            return hit
        self.built.append(tuple(w.clone() for w in weights))
        return self._cache_put(key, weights, ('planes', len(self.built)))

    def folded_planes(self, layer):
        wq = self._folded_weight('q', layer.k_proj.weight, layer.q_proj.weight)
        wm = self._folded_weight('m', layer.merge.weight, layer.v_proj.weight)
        return wq, wm, self.weight_planes((wq,)), self.weight_planes((wm,))


def _layer(seed=7):
    net = FeatureTransformer()
    net.load_state_dict(_weights(seed))
    return net, net.layers[2].cross_attn_ffn


def test_folded_planes_are_cached_and_rebuilt_with_the_weights():
    ops = _Recorder()
    net, layer = _layer()
    wq, wm, pq, pm = ops.folded_planes(layer)
    assert torch.equal(wq, fold_weights('q', layer.k_proj.weight, layer.q_proj.weight))
    assert torch.equal(wm, fold_weights('m', layer.merge.weight, layer.v_proj.weight))
    assert len(ops.built) == 2 and torch.equal(ops.built[0][0], wq) and torch.equal(ops.built[1][0], wm)
    gen = ops.cache_generation
    again = ops.folded_planes(layer)                               # a second forward: nothing is built, the generation stands still
    assert again[0] is wq and again[1] is wm and again[2] is pq and again[3] is pm
    assert len(ops.built) == 2 and ops.cache_generation == gen     # (the two-part first-call rule reads the generation)

    # load_state_dict copies in place through autograd-visible ops: the version moves, no call is needed
    net.load_state_dict(_weights(seed=8))
    wq2, wm2, pq2, pm2 = ops.folded_planes(layer)
    assert wq2 is not wq and not torch.equal(wq2, wq) and torch.equal(wq2, fold_weights('q', layer.k_proj.weight, layer.q_proj.weight))
    assert torch.equal(wm2, fold_weights('m', layer.merge.weight, layer.v_proj.weight))
    assert len(ops.built) == 4 and pq2 != pq and pm2 != pm and ops.cache_generation > gen

    # an in-place edit of ONE of the two factors through .data is invisible (no version, same address): invalidate_weights()
    layer.v_proj.weight.data.mul_(2.0)
    assert ops.folded_planes(layer)[1] is wm2                      # (documented: stale until told)
    ops.invalidate_weights()
    wq3, wm3, _, _ = ops.folded_planes(layer)
    assert torch.equal(wm3, fold_weights('m', layer.merge.weight, layer.v_proj.weight)) and not torch.equal(wm3, wm2)
    assert torch.equal(wq3, wq2) and wq3 is not wq2 and len(ops.built) == 6

    # a visible in-place edit of the OTHER factor (k_proj, which only the folded query weight reads) rebuilds that one alone
    with torch.no_grad():
        layer.k_proj.weight.mul_(0.5)
    wq4, wm4, _, _ = ops.folded_planes(layer)
    assert wm4 is wm3 and not torch.equal(wq4, wq3) and len(ops.built) == 7


def test_set_precision_drops_the_backend_with_its_folded_planes():
    model = UniMatch()
    model._ops = ops = _Recorder()
    ops.folded_planes(model.transformer.layers[0].self_attn)
    assert len(ops._wcache) == 4
    model.set_precision('fast')
    assert model._ops is None                                      # the next forward builds a fresh HipOps: nothing of the old mode survives
    model._ops = ops
    model.invalidate_weights()
    assert not ops._wcache


def test_ffn_planes_entry_point_refuses_bad_arguments_before_any_launch():
    import ctypes
    from unimatch_amd import _abi
    lib = _abi.load()
    fake = ctypes.c_void_p(256)
    assert lib.um_ffn_planes_fwd(fake, fake, fake, fake, 128, 64, 10, fake, fake, 1e-5, fake, None, 0, None, 0, None) == -1
    assert lib.um_ffn_planes_fwd(fake, fake, fake, fake, 0, 64, 10, fake, fake, 1e-5, fake, fake, 0, None, 0, None) == -1
    assert lib.um_ffn_planes_fwd(fake, fake, fake, fake, 128, 48, 10, fake, fake, 1e-5, fake, fake, 0, None, 0, None) == -1


def test_the_knob_is_a_class_attribute_and_prices_no_projection_flops():
    """bench.py --set flips class attributes of HipOps; its FFN roofline adds the k | v projection FLOPs when block_kv, fused_kv,
    fused_ffn, fused_qproj and fused_merge are all set -- with the fold on the FFN launches execute none."""
    assert HipOps.fold_kv is True
    assert not all(getattr(HipOps, k) for k in ('block_kv', 'fused_kv', 'fused_ffn', 'fused_qproj', 'fused_merge'))
