"""HIP-graph replay of the whole forward.

The forward of ``UniMatch`` is a fixed sequence of ~200 kernel launches with no host synchronisation (the
reference's per-layer device->host sync, transformer.py:55, is gone), so for a fixed input shape it can be captured
once and replayed: at small batch the step is launch-bound (about 10 us of host time per launch), which is the
regime of the reference's own evaluation protocol (batch 1).  ``GraphedUniMatch(model)`` behaves like the model;
each distinct (shapes, keyword arguments) combination is captured on first use.

A capture freezes the ADDRESSES of the weights' operand planes (buffers of ``HipOps._wcache``), while biases and LayerNorm
parameters are read in place.  A graph is therefore valid for one state of the weights only -- the parameters' identity, address,
version and dtype, the backend object and its ``cache_generation`` (which moves whenever a cache entry is built or the cache is
dropped: ``invalidate_weights``, the prune) -- and is captured again, once, when that state has moved: after ``load_state_dict``,
an in-place edit, ``.to()``, ``set_precision``.  Superseded graphs are released with their private pools and workspaces.
"""
import contextlib
import warnings

import torch


def _freeze(v):
    if isinstance(v, (list, tuple)):
        return tuple(_freeze(x) for x in v)
    if torch.is_tensor(v):
        return ('tensor', tuple(v.shape), str(v.dtype))
    return v


def _find_ops(model):
    """The ``HipOps`` of a model, looked for through wrappers (``ShardedUniMatch(model)``, ``DistributedDataParallel`` ...: the
    attributes ``model`` / ``module``), so that the capture's scope reaches the instance whose workspaces it bakes in."""
    seen = set()
    while model is not None and id(model) not in seen:
        seen.add(id(model))
        ops = getattr(model, 'ops', None)
        if ops is not None and hasattr(ops, 'graph_scope'):
            return ops
        model = getattr(model, 'model', None) or getattr(model, 'module', None)
    return None


def _find_weights_state(model):
    """``UniMatch.weights_state`` of the model inside the same wrappers; a module without one is walked parameter by parameter."""
    seen, outer = set(), model
    while model is not None and id(model) not in seen:
        seen.add(id(model))
        fn = getattr(model, 'weights_state', None)
        if fn is not None:
            return fn()
        model = getattr(model, 'model', None) or getattr(model, 'module', None)
    if hasattr(outer, 'parameters'):
        return tuple((id(p), p.data_ptr(), p._version, p.dtype) for p in outer.parameters())
    return None


class GraphedUniMatch(torch.nn.Module):
    def __init__(self, model, warmup=2, clone_output=True):
        super().__init__()
        self.model = model
        self.warmup = warmup
        self.clone_output = clone_output
        self._graphs = {}

    def _capture(self, img0, img1, kw):
        static = {'img0': img0.clone(), 'img1': img1.clone(),
                  'kw': {k: (v.clone() if torch.is_tensor(v) else v) for k, v in kw.items()}}
        # The scratch buffers the forward bakes in (split-launch arrival counters that must be zero between launches, activation
        # planes) are allocated and zeroed by the eager warm-up OUTSIDE the capture under this graph's scope, and the graph then
        # owns them alone: two graphs replayed concurrently share no counter, and an aborted capture's buffers are dropped.
        ops = _find_ops(self.model)
        with ops.graph_scope(object()) if ops is not None else contextlib.nullcontext({}) as owned:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):           # warm-up: position tables, weight planes, split workspaces
                for _ in range(max(1, self.warmup)):
                    self.model(static['img0'], static['img1'], **static['kw'])
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static['out'] = self.model(static['img0'], static['img1'], **static['kw'])['flow_preds'][0]
        static['graph'] = graph
        static['workspaces'] = owned                # alive as long as the graph
        static['state'] = self._state()             # after the warm-up: building the planes moved the cache generation
        return static

    def _state(self):
        """What a captured graph is valid for besides its key (see the module's docstring)."""
        ops = _find_ops(self.model)
        return (_find_weights_state(self.model), id(ops), getattr(ops, 'cache_generation', None))

    def _release_superseded(self, state):
        """Forget every graph of another weight state: nothing may replay it again, and its pool, static tensors and workspaces
        would otherwise stay allocated until its own configuration is called the next time."""
        for key in [k for k, e in self._graphs.items() if e is not False and e['state'] != state]:
            del self._graphs[key]

    def forward(self, img0, img1, **kw):
        if not img0.is_cuda:
            return self.model(img0, img1, **kw)
        key = (tuple(img0.shape), tuple(img1.shape), str(img0.dtype), tuple(sorted((k, _freeze(v)) for k, v in kw.items())))
        entry = self._graphs.get(key)
        if entry:
            state = self._state()
            if entry['state'] != state:
                entry = None
                self._release_superseded(state)
        if entry is None:
            try:
                entry = self._capture(img0, img1, kw)
            except RuntimeError as exc:          # an op that cannot be captured (e.g. a library call that syncs)
                warnings.warn(f'HIP graph capture failed ({exc}); running eagerly for this configuration')
                entry = False
                # an aborted capture leaves the stream in an invalidated capture state and may have filled the model's
                # operand-plane caches from the graph's private memory pool: drain the device and forget them
                torch.cuda.synchronize()
                if hasattr(self.model, 'invalidate_weights'):
                    self.model.invalidate_weights()
            self._graphs[key] = entry
        if entry is False:
            return self.model(img0, img1, **kw)
        entry['img0'].copy_(img0)
        entry['img1'].copy_(img1)
        for k, v in kw.items():
            if torch.is_tensor(v):
                entry['kw'][k].copy_(v)
        entry['graph'].replay()
        out = entry['out']
        return {'flow_preds': [out.clone() if self.clone_output else out]}
