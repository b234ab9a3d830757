"""Shared by tests/test_weight_cache_gpu.py and tests/test_weight_cache_cpu.py: everything about ``HipOps._wcache`` that needs no GPU.

The hot path never reads an ``nn.Parameter``: it reads derived copies (operand planes, folded / padded / packed weights) that
``HipOps`` caches under ``(tag, (id, _version, data_ptr, device, dtype) per tensor)``.  A cache entry that outlives a change of its
weights gives the right kernel's result for the wrong weights, which no comparison on freshly built weights can see.
"""
import ast
import pathlib

import torch

PACKAGE = pathlib.Path(__file__).resolve().parent.parent / 'unimatch_amd'

# Every kind of entry in HipOps._wcache.  A tuple tag -- ('conv7', stride), ('padw', cin_to), ('refine', name) -- counts by its
# first element.  A new cache site fails test_weight_cache_cpu.py until it is listed here, and the GPU file fails until one of its
# setups reaches it.
CACHE_TAGS = frozenset({'lin', 'fold_q', 'fold_m', 'kv4', 'conv', 'conv7', 'stem', 'padw', 'refine'})

# (config, HipOps attributes, parameter-name prefix of the sweep).  The refinement block prepares its weights differently for 2 and
# 1 flow channels and for bilinear_up: all three refinement configs.  fold_kv off reaches 'kv4' and the unfolded 'lin' groups.
SETUPS = {
    'gmflow_s1': ('gmflow_s1', {}, ''),
    'gmflow_s2_rr6': ('gmflow_s2_rr6', {}, ''),
    'gmstereo_s2_rr3': ('gmstereo_s2_rr3', {}, ''),
    'gmdepth_s1_rr1': ('gmdepth_s1_rr1', {}, ''),
    'gmflow_s1-unfolded': ('gmflow_s1', {'fold_kv': False}, 'transformer.'),
    'gmflow_s1-unfolded-fused_kv': ('gmflow_s1', {'fold_kv': False, 'fused_kv': True}, 'transformer.'),
}
PARAMETER_COUNTS = {'gmflow_s1': 123, 'gmflow_s2_rr6': 152, 'gmstereo_s2_rr3': 152, 'gmdepth_s1_rr1': 151}

# Parameters whose perturbation leaves the prediction bitwise unchanged on the TRUSTED path (invalidate_weights() before the
# forward), one reason each: the head or branch the config does not run.  gmflow_s1: none (each of its 123 parameters also changes
# the CPU oracle's output bitwise under this perturbation).
NO_EFFECT = {
    'gmflow_s1': {},
    'gmflow_s2_rr6': {},
    'gmstereo_s2_rr3': {},
    'gmdepth_s1_rr1': {},
}


def tag_kind(tag):
    return tag[0] if isinstance(tag, tuple) else tag


def cache_kinds(ops):
    """The kinds of entry a backend's weight cache holds now."""
    return {tag_kind(key[0]) for key in ops._wcache}


def perturb_(p, generator):
    """The sweep's edit: in place, visible to autograd's version counter, about 5 % of the parameter's mean magnitude."""
    noise = torch.randn(p.shape, generator=generator)
    with torch.no_grad():
        p.add_(noise.to(p.device) * (0.05 * p.abs().mean() + 1e-3))


# ------------------------------------------------------------------------------------------------ the call sites, read from the source
def _calls(tree, name):
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == name:
            yield node


def _literal_kind(node):
    """The kind of a tag expression: 'lin', ('conv7', stride) -> 'conv7', 'fold_' + kind -> 'fold_*'."""
    if isinstance(node, ast.Constant) and isinstance(node.value, str):
        return node.value
    if isinstance(node, ast.Tuple) and node.elts and isinstance(node.elts[0], ast.Constant):
        return node.elts[0].value
    if isinstance(node, ast.BinOp) and isinstance(node.op, ast.Add) and isinstance(node.left, ast.Constant):
        return node.left.value + '*'
    return ast.dump(node)                                           # anything else is reported as it is: the comparison fails


def cache_sites():
    """``[(file, line, kind)]`` of every ``_cache_get(tag, tensors)`` call of the package.  ``'fold_' + kind`` is expanded with the
    kinds that the package's own ``_folded_weight(kind, a, b)`` calls pass."""
    sites, fold_kinds = [], set()
    trees = {p: ast.parse(p.read_text()) for p in sorted(PACKAGE.glob('*.py'))}
    for tree in trees.values():
        for call in _calls(tree, '_folded_weight'):
            first = call.args[0]
            fold_kinds.add(first.value if isinstance(first, ast.Constant) else ast.dump(first))
    for path, tree in trees.items():
        for call in _calls(tree, '_cache_get'):
            kind = _literal_kind(call.args[0])
            for k in ([kind[:-1] + f for f in sorted(fold_kinds)] if kind.endswith('*') else [kind]):
                sites.append((path.name, call.lineno, k))
    return sites


# ------------------------------------------------------------------------------------------------ NhwcUpdateBlock._w keys vs what build() reads
class RecordingBackend:
    """The two backend methods ``NhwcUpdateBlock._w`` uses, without a GPU: nothing is ever cached, so every ``build`` runs."""

    def __init__(self):
        self.calls = []                                             # (tag, ids of the key tensors)

    def _cache_get(self, tag, tensors):
        self.calls.append((tag, tuple(id(t) for t in tensors)))
        return (tag, len(self.calls)), None

    def _cache_put(self, key, tensors, value):
        return value

    def conv_weight_planes_from(self, weight):
        return ('planes', tuple(weight.shape))


def refine_key_audit(model):
    """Run the refinement block's weight preparation on the CPU with every parameter access traced ->
    ``[(tag, parameters build() read, parameters in the key)]`` by name.

    The trace: for the time of each ``_w`` call, ``nn.Module.__getattr__`` -- the one door to a module's parameters -- notes which
    parameter objects it hands out.  ``_w`` evaluates its ``params`` list before it is entered, so all that is noted inside is what
    ``build`` reads."""
    from unimatch_amd.refine_nhwc import NhwcUpdateBlock
    names = {id(p): n for n, p in model.named_parameters()}
    backend = RecordingBackend()
    block = NhwcUpdateBlock(backend, model.refine, model.refine_proj)
    report, reads = [], None
    plain_getattr = torch.nn.Module.__getattr__
    plain_w = NhwcUpdateBlock._w

    def traced_getattr(module, name):
        value = plain_getattr(module, name)
        if reads is not None and id(value) in names:
            reads.add(names[id(value)])
        return value

    def traced_w(self, tag, params, build):
        nonlocal reads
        reads = set()
        try:
            out = plain_w(self, tag, params, build)
        finally:
            seen, reads = reads, None
        report.append((tag, seen, {names[id(p)] for p in params}))
        return out

    torch.nn.Module.__getattr__ = traced_getattr
    NhwcUpdateBlock._w = traced_w
    try:
        block._weights()
    finally:
        torch.nn.Module.__getattr__ = plain_getattr
        NhwcUpdateBlock._w = plain_w
    assert [c[0] for c in backend.calls] == [('refine', tag) for tag, _, _ in report]
    return report
