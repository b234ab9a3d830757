"""The weight caches of the hot path, as far as they can be checked without a GPU (tests/weight_cache_util.py has the why).

* every ``_cache_get`` call site of the package has a tag that tests/test_weight_cache_gpu.py sweeps;
* every ``NhwcUpdateBlock._w(tag, params, build)`` keys on all the parameters its ``build`` reads;
* the forward refuses parameters that are not fp32 (biases and LayerNorm parameters reach the kernels as raw addresses).
"""
import pytest
import torch

from tests.weight_cache_util import CACHE_TAGS, NO_EFFECT, PARAMETER_COUNTS, SETUPS, cache_sites, refine_key_audit
from unimatch_amd import UniMatch
from unimatch_amd.synth import CONFIGS


def test_every_cache_site_has_a_swept_tag():
    """A new ``_cache_get`` call (or a tag that no longer exists) fails here until CACHE_TAGS -- and with it the GPU sweeps, whose
    observed tags must equal CACHE_TAGS -- follows."""
    sites = cache_sites()
    print('\n'.join(f'{f}:{line}  {kind}' for f, line, kind in sites))
    assert len(sites) >= 9
    assert {kind for _, _, kind in sites} == set(CACHE_TAGS), sites


@pytest.mark.parametrize('name', ['gmflow_s2_rr6', 'gmstereo_s2_rr3', 'gmdepth_s1_rr1'])
def test_refinement_weight_keys_name_every_parameter_their_build_reads(name):
    """2 flow channels with a mask head, 1 flow channel with one, 1 flow channel with bilinear_up (no mask head)."""
    model = UniMatch(**CONFIGS[name][0]).eval()
    report = refine_key_audit(model)
    tags = [tag for tag, _, _ in report]
    # 5 (projection, motion encoder) + 2 passes x 6 gate forms + 2 (flow head) + 2 (mask head, absent with bilinear_up)
    assert len(tags) == len(set(tags)) and len(tags) == (21 if model.refine.mask is not None else 19), tags
    for tag, read, keyed in report:
        assert read, (tag, 'the trace saw no parameter access: the audit itself is broken')
        assert read <= keyed, f"('refine', {tag!r}): build() reads {sorted(read - keyed)}, which the key does not hold"
    # every parameter of the block reaches the kernels through one of these entries, or directly (convf1: HipOps.conv7's own entry)
    covered = set().union(*(keyed for _, _, keyed in report))
    block = {n for n, _ in model.named_parameters() if n.startswith(('refine.', 'refine_proj.'))}
    assert block - covered == {'refine.encoder.convf1.weight', 'refine.encoder.convf1.bias'}


def test_the_setups_of_the_gpu_sweeps_are_the_configs_they_claim():
    for name, count in PARAMETER_COUNTS.items():
        model = UniMatch(**CONFIGS[name][0])
        names = [n for n, _ in model.named_parameters()]
        assert len(names) == count
        assert set(NO_EFFECT[name]) <= set(names)                   # an exemption names a parameter that exists
        assert all(isinstance(reason, str) and len(reason) > 20 for reason in NO_EFFECT[name].values())
    assert NO_EFFECT['gmflow_s1'] == {}
    for config, flags, prefix in SETUPS.values():
        assert config in PARAMETER_COUNTS and (prefix == '') == (not flags)


def test_forward_refuses_parameters_that_are_not_fp32():
    """``model.half()`` (or one bias converted by hand) must be refused by name before any launch: the kernels would read an fp16
    bias as fp32, past its end.  The check is called directly: it is what every CUDA entry point runs first."""
    model = UniMatch(**CONFIGS['gmflow_s2_rr6'][0]).eval()
    model.check_parameter_dtypes()
    bias = model.refine_proj.bias
    bias.data = bias.data.half()
    with pytest.raises(ValueError, match='float32.*bias.*float16'):
        model.check_parameter_dtypes()
    bias.data = bias.data.float()
    model.check_parameter_dtypes()
    model.half()                                                    # (_apply: the parameter dicts are collected again)
    with pytest.raises(ValueError, match='float32'):
        model.check_parameter_dtypes()
    model.float()
    model.transformer.layers[0].self_attn.norm1.weight = torch.nn.Parameter(torch.ones(128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match='bfloat16'):               # a parameter assigned anew is seen without a rescan
        model.check_parameter_dtypes()
    # every CUDA entry point runs the check before it touches the backend's kernels
    import inspect
    for fn in (UniMatch._forward_one, UniMatch.forward_sequence, UniMatch._depth_sequence, UniMatch.forward_multiview, UniMatch.predict):
        assert 'self.check_parameter_dtypes()' in inspect.getsource(fn), fn.__name__
