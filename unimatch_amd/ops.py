"""Typed Python wrappers over the C ABI: one method per reference hot-path function.

``HipOps`` is the ONLY implementation of the hot path that the product ships.  Every method checks
shapes / dtypes / contiguity, allocates the output (and scratch workspace) as torch tensors, and enqueues
the HIP kernels on torch's current stream through ``ctypes``.  Feature tensors are token-major
``[N, L, C]`` fp32 (C = 128); flow-like tensors are ``[N, V, h, w]`` fp32 as in the reference.
"""
import contextlib
import ctypes
import threading
import weakref
from collections import namedtuple

import torch

from . import _abi

PRECISIONS = {'exact': _abi.MODE_EXACT, 'fast': _abi.MODE_FAST}


class KernelTimer:
    """Optional per-launch HIP-event timing on the stream the kernels are launched on."""

    def __init__(self):
        self.records = []          # (name, start_event, end_event, meta)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, s, e, meta in self.records:
            d = out.setdefault(name, {'calls': 0, 'ms': 0.0, 'meta': meta})
            d['calls'] += 1
            d['ms'] += s.elapsed_time(e)
        return out


def _ptr(t):
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check_tokens(name, t, n=None, tokens=None):
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous()):
        raise ValueError(f'{name}: expected a contiguous CUDA float32 [N, L, C] tensor, got '
                         f'{tuple(t.shape)} {t.dtype} {t.device} contiguous={t.is_contiguous()}')
    if n is not None and t.shape[0] != n or tokens is not None and t.shape[1] != tokens:
        raise ValueError(f'{name}: shape {tuple(t.shape)} does not match N={n}, L={tokens}')


def _check_map(name, t, n, h, w):
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()
            and t.shape[0] == n and t.shape[2] == h and t.shape[3] == w):
        raise ValueError(f'{name}: expected a contiguous CUDA float32 [{n}, V, {h}, {w}] tensor, got '
                         f'{tuple(t.shape)} {t.dtype}')


def pack_kv4_weights(weights):
    """The four ``[128, 128]`` projection weights (k_self, v_self, k_cross, v_cross) packed as the ``[256, 256]`` matrix
    ``um_kv4_fwd`` / ``um_ffn_kv_fwd`` stream like a W1 slice of the FFN: row ``32 c + r`` (chunk c = 0..7, r = 0..31) carries
    ``W4[32 c + r]`` in columns 0..127 (the rows role 0 of a wave pair multiplies: k_self | v_self) and ``W4[256 + 32 c + (r ^ 16)]``
    in columns 128..255 (role 1 reads ring rows permuted by ^16: k_cross | v_cross), ``W4`` = the four weights stacked."""
    w4 = torch.cat([w.detach().float() for w in weights], 0)                         # [512, 128]
    perm = torch.arange(32, device=w4.device) ^ 16
    cross = w4[256:].view(8, 32, 128)[:, perm].reshape(256, 128)
    return torch.cat([w4[:256], cross], 1).contiguous()


def fold_weights(kind, a, b):
    """The folded ``[128, 128]`` weight of one attention layer, formed in fp64 and rounded once to fp32.  The layer is single-head, its
    Linears are bias-free and nothing non-linear sits between the projections and the attention (transformer.py:23-27, 58-60, 137), so
    ``(x Wq^T)(y Wk^T)^T = (x (Wk^T Wq)^T) y^T`` and ``merge(P (y Wv^T)) = (P y)(Wm Wv)^T``:
    ``kind='q'``: ``a, b = Wk, Wq -> Wk^T Wq``;  ``kind='m'``: ``a, b = Wm, Wv -> Wm Wv``.  Sum over the middle index without a BLAS call."""
    a, b = a.detach().double(), b.detach().double()
    if kind == 'q':
        a = a.t()
    elif kind != 'm':
        raise ValueError(f"fold_weights: kind must be 'q' or 'm', got {kind!r}")
    return (a.unsqueeze(2) * b.unsqueeze(0)).sum(1).float().contiguous()


WorkspaceKey = namedtuple('WorkspaceKey', 'kind geometry device owner')


class _Scope(threading.local):
    token = None               # the graph being warmed up / captured on this thread (graph_scope)
    lane = 0                   # the part of a batch being enqueued on this thread (part_scope)


class WorkspaceRegistry:
    """Scratch that a launch finds zeroed -- split small launches' partials + arrival counters, the refinement block's activation
    planes -- one buffer per ``WorkspaceKey``: ``kind`` ``'attn_ksplit'`` / ``'ffn_hsplit'`` / ``('planes', tag)``, ``geometry`` the
    arguments of its size query, ``owner`` the current stream (launches in flight on two streams share no counter) or, inside the
    thread-local :meth:`graph_scope` / :meth:`part_scope`, ``(graph token, lane)``: the eager warm-up allocates and zeroes a graph's
    buffers OUTSIDE the capture, every graph and every part of a captured forward has its own.  A request inside a capture with no
    buffer of its key gets a capture-private zeroed one (a memset node of the graph) that is never cached.  ``stream`` and
    ``capturing`` are injectable: the bookkeeping runs without a GPU."""

    GEOMETRIES = 8             # split workspaces kept per (kind, device, owner), oldest dropped first

    def __init__(self, stream=None, capturing=None):
        self._entries = {}
        self._scope = _Scope()
        self._stream_handle = stream or _stream
        self._capturing = capturing or torch.cuda.is_current_stream_capturing

    @contextlib.contextmanager
    def graph_scope(self, token):
        """Requests inside are owned by ``token``; on exit, exceptions included, its buffers leave the registry into the yielded
        dict, which the graph keeps alive (an aborted capture's are dropped with it)."""
        prev, self._scope.token = self._scope.token, token
        owned = {}
        try:
            yield owned
        finally:
            self._scope.token = prev
            for k in [k for k in self._entries if isinstance(k.owner, tuple) and k.owner[0] is token]:
                owned[k] = self._entries.pop(k)

    @contextlib.contextmanager
    def part_scope(self, lane):
        prev, self._scope.lane = self._scope.lane, lane
        try:
            yield
        finally:
            self._scope.lane = prev

    def workspace_scope(self):
        return self._scope.token, self._scope.lane

    def workspace_entries(self):
        """``[(WorkspaceKey, buffer), ...]``: a read-only view for tests."""
        return list(self._entries.items())

    def _workspace(self, kind, geometry, nbytes, device, keep):
        scope = self._scope
        owner = self._stream_handle() if scope.token is None else (scope.token, scope.lane)
        buf = self._entries.get((kind, geometry, device, owner))         # (a plain tuple hashes and compares as the key does)
        if buf is None:
            if self._capturing():
                return torch.zeros(nbytes, dtype=torch.uint8, device=device)
            group = [k for k in self._entries if (k.kind, k.device, k.owner) == (kind, device, owner)]
            for k in group[:max(0, len(group) + 1 - keep)]:
                del self._entries[k]
            buf = self._entries[WorkspaceKey(kind, geometry, device, owner)] = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        return buf

    def release_cached_planes(self):
        """Drop every cached activation-plane buffer (~590 MB per stream at config 4; captured graphs keep their own).  Safe at any
        time between forwards: the next forward allocates and zeroes a fresh set."""
        for k in [k for k in self._entries if isinstance(k.kind, tuple)]:
            del self._entries[k]


class HipOps(WorkspaceRegistry):
    """The hot path on MI355X.  ``precision``: 'exact' (fp16 hi+lo split MFMA operands) or 'fast' (bf16)."""

    fused_tail = True          # Transformer-layer linears / LayerNorm / GELU / residual run on um_linear_fwd
    fused_ffn = True           # ... and the FFN as one kernel (um_ffn_fwd) instead of two um_linear_fwd launches
    fused_merge = True         # merge + LayerNorm (+ residual) in the attention kernel's epilogue
    fused_qproj = True         # ... and the query projection in its prologue (um_window_attn_qproj_merge_fwd)
    block_kv = True            # one k | v projection launch per Transformer block (both layers' keys / values: um_kv4_fwd)
    refine_hoist = True        # refinement loop: the iteration-invariant share of the GRU gate convolutions computed once per scale
    fused_kv = False           # ... which, from block 1 on, is the previous block's FFN epilogue (um_ffn_kv_fwd): no launch at all.
                               #     block_kv / fused_kv only act with fold_kv off; fold_kv = 0 with fused_kv = 1 is the forward before the fold
                               #     (off by default because bench.py prices the FFN launches' k | v FLOPs by this attribute)
    fold_kv = True             # k_proj / v_proj folded into the query and merge weights (q' = Wk^T Wq, merge' = Wm Wv, fold_weights): keys =
                               #     values = the token stream itself, one [NS][M][128] planes tensor per block, written by the previous
                               #     block's FFN launch (um_ffn_planes_fwd) or, for block 0, by one format pass
    # (class attributes: tests and tools/ab_bench.py flip them programmatically; the product reads no environment variable)
    fused_conv = True          # encoder convolutions + InstanceNorm in NHWC on um_conv2d_fwd / um_nhwc_instance_norm
    norm_on_load = True        # ... a residual block's middle InstanceNorm + ReLU inside its second convolution (um_conv2d_norm_fwd)
    fused_entry = True         # ... a stride-2 block's input apply, first convolution and projection shortcut in one launch (um_conv2d_entry_fwd),
                               #     and the projection's own InstanceNorm inside the block's output apply (um_nhwc_instance_norm_sc)
    fused_glue = True          # no copy / add / format pass between neighbouring kernels: the stem reads the two image tensors of a pair batch
                               #     (um_stem_conv_pair_fwd), the encoder's last convolution adds the position table (um_conv2d_addend_fwd), the
                               #     upsampler head's input is one launch (um_nhwc_concat_planes) and its hidden map stays operand planes, the
                               #     parts of a batch write into one prediction (convex_upsample(out=))
    CONV_MODE = 0              # ... always in the exact arithmetic: 'fast' (bf16) is a property of the matching path only
    WSHIFT = 10                # weights are scaled by 2^10 before the fp16 split (exact), see linear.hip

    def __init__(self, precision='exact'):
        if precision not in PRECISIONS:
            raise ValueError(f'precision must be one of {sorted(PRECISIONS)}')
        self.lib = _abi.load()                # raises HipExtensionError when the library is missing
        if not torch.cuda.is_available():
            raise _abi.HipExtensionError('no GPU visible: the UniMatch hot path only runs on the HIP extension')
        self.precision = precision
        self.mode = PRECISIONS[precision]
        self.timer = None                     # set to a KernelTimer() to time launches with HIP events
        self.nplanes = 2 if precision == 'exact' else 1
        self._wcache = {}                     # weight planes, keyed by the identity + version of the fp32 tensors
        self.cache_generation = 0             # counts builds of shared cache entries (streams.PartRunner)
        WorkspaceRegistry.__init__(self)

    # ------------------------------------------------------------------ helpers
    def _ws(self, nbytes, device):
        return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)

    def _launch(self, name, fn, meta=None):
        if self.timer is None:
            return fn()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        r = fn()
        e.record()
        self.timer.records.append((name, s, e, meta))
        return r

    # ------------------------------------------------------------------ attention
    def window_attention(self, q, k, v, h, w, win_h, win_w, shift_h=0, shift_w=0):
        """softmax(q k^T/sqrt(C) + shift mask) v inside windows; q, k, v ``[S, h*w, C]``."""
        s, l, c = q.shape
        _check_tokens('q', q, tokens=h * w)
        _check_tokens('k', k, s, l)
        _check_tokens('v', v, s, l)
        out = torch.empty_like(q)
        nbytes = self.lib.um_window_attn_workspace_bytes(s, l, c, self.mode)
        ws = self._ws(nbytes, q.device)
        n = win_h * win_w
        meta = {'flops': 4.0 * s * l * n * c, 'bytes': 4.0 * 4 * s * l * c}
        code = self._launch('window_attn', lambda: self.lib.um_window_attn_fwd(
            _ptr(q), _ptr(k), _ptr(v), _ptr(out), s, h, w, c, win_h, win_w, shift_h, shift_w,
            self.mode, _ptr(ws), ws.numel(), _stream()), meta)
        _abi.check(code, 'um_window_attn_fwd')
        return out

    # ------------------------------------------------------------------ fused Transformer-layer tail
    def _cache_get(self, tag, tensors):
        """Cached value for these tensor OBJECTS at their current versions.  Keyed by identity and validated through weak
        references: a ``data_ptr`` key is wrong for temporaries (the allocator hands a freed weight's address to the next
        tensor of the same shape)."""
        # identity + autograd version + storage address + device + dtype: `p.data = ...`, `.to(device)`, `.float()` keep id and
        # version but move / retype the storage; an IN-PLACE edit through `.data` (`p.data.mul_(2)`) changes none of these and
        # needs invalidate_weights() (UniMatch.invalidate_weights(), or check_weights=True for a per-forward fingerprint)
        key = (tag,) + tuple((id(t), t._version, t.data_ptr(), str(t.device), t.dtype) for t in tensors)
        hit = self._wcache.get(key)
        if hit is not None and all(r() is t for r, t in zip(hit[0], tensors)):
            return key, hit[1]
        return key, None

    def invalidate_weights(self):
        """Forget every cached operand plane (call after editing weights in place through ``.data``) and every split
        workspace (a launch that was cut short -- aborted capture, device error -- may have left arrival counters non-zero)."""
        self._wcache.clear()
        self._entries.clear()
        self.cache_generation += 1

    def _cache_put(self, key, tensors, value):
        if len(self._wcache) > 256:
            self._wcache = {k: v for k, v in self._wcache.items() if all(r() is not None for r in v[0])}
            if len(self._wcache) > 256:
                self._wcache.clear()
        self._wcache[key] = (tuple(weakref.ref(t) for t in tensors), value)
        # counts the builds of shared (stream-independent) cache entries: ConcurrentUniMatch only runs its parts on separate streams
        # when the previous forward built none -- an entry is written on the stream that first needs it
        self.cache_generation += 1
        return value

    def weight_planes(self, weights):
        """MFMA operand planes of ``cat(weights, 0)`` ([N, K] fp32 each, same K), cached until a weight changes."""
        key, hit = self._cache_get('lin', weights)
        if hit is not None:
            return hit
        w = (weights[0] if len(weights) == 1 else torch.cat(list(weights), 0)).detach().float().contiguous()
        n, k = w.shape
        self._check_weight_range(w, self.WSHIFT if self.mode == 0 else 0, 'Linear weight')
        planes = torch.empty(self.lib.um_planes_bytes(n, k, self.mode), dtype=torch.uint8, device=w.device)
        _abi.check(self.lib.um_weight_planes(_ptr(w), _ptr(planes), n, k, self.WSHIFT, self.mode, _stream()),
                   'um_weight_planes')
        return self._cache_put(key, weights, (planes, n, k))

    def _folded_weight(self, kind, a, b):
        """:func:`fold_weights` of the two parameters, cached like their planes (identity + version; ``invalidate_weights``).  The planes
        of the result come from :meth:`weight_planes`, keyed by this tensor: they live exactly as long as this entry."""
        key, hit = self._cache_get('fold_' + kind, (a, b))
        if hit is not None:
            return hit
        if tuple(a.shape) != (128, 128) or tuple(b.shape) != (128, 128):
            raise ValueError('folded attention weights: expected two [128, 128] weights')
        return self._cache_put(key, (a, b), fold_weights(kind, a, b))

    @staticmethod
    def _check_weight_range(w, shift, what):
        """Exact mode stores weights as fp16 hi + lo planes of ``w * 2^shift``: anything at or above 65504 / 2^shift would become
        inf in the hi plane (and NaN in the output) without a message.  One-time check per cached weight (synchronises once)."""
        limit = 65504.0 / float(1 << shift)
        amax = float(w.abs().max()) if w.numel() else 0.0
        if not amax < limit:
            raise ValueError(f'{what}: max |w| = {amax:.4g} does not fit the fp16 operand planes (|w| < {limit:.4g} at the '
                             f'2^{shift} pre-scale; see include/unimatch_hip.h, "Operand range")')

    def _check_rows(self, name, t, k):
        if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous() and t.shape[1] == k):
            raise ValueError(f'{name}: expected a contiguous CUDA float32 [M, {k}] tensor, got {tuple(t.shape)} {t.dtype}')

    def linear_planes(self, a, weights, a1=None, gelu=False, a_planes_k=None):
        """``(gelu)(A . cat(weights)^T)`` written as MFMA operand planes ``[NS][M][N]`` (flat uint8 tensor).

        A is ``a`` fp32 ``[M, K]``, or the K-concatenation of ``a`` and ``a1`` (``[M, K/2]`` each), or -- with
        ``a_planes_k`` -- ``a`` is already a plane tensor with K = a_planes_k columns.  ``weights = ()``: the identity -- the planes
        of ``a`` itself, one format pass (``um_weight_planes`` at scale 1): the key / value operand of the folded attention."""
        if len(weights) == 0:
            if a1 is not None or gelu or a_planes_k is not None or not (a.dim() == 2 and a.shape[0] > 0):
                raise ValueError('linear_planes: the identity takes one fp32 [M, K] tensor and no epilogue')
            m, k = a.shape
            self._check_rows('a', a, k)
            out = torch.empty(self.lib.um_planes_bytes(m, k, self.mode), dtype=torch.uint8, device=a.device)
            _abi.check(self._launch('split_planes', lambda: self.lib.um_weight_planes(_ptr(a), _ptr(out), m, k, 0, self.mode, _stream())),
                       'um_weight_planes')
            return out, m, k
        wp, n, k = self.weight_planes(weights)
        if a_planes_k is not None:
            m = a.numel() // (2 * self.nplanes * a_planes_k)
            args = (None, None, _ptr(a))
        else:
            m = a.shape[0]
            self._check_rows('a', a, k // 2 if a1 is not None else k)
            if a1 is not None:
                self._check_rows('a1', a1, k // 2)
            args = (_ptr(a), _ptr(a1) if a1 is not None else None, None)
        out = torch.empty(self.lib.um_planes_bytes(m, n, self.mode), dtype=torch.uint8, device=a.device)
        meta = {'flops': 2.0 * m * n * k}
        code = self._launch('linear', lambda: self.lib.um_linear_fwd(
            args[0], args[1], args[2], _ptr(wp), m, n, k, self.WSHIFT, 2 if gelu else 0, _ptr(out),
            None, None, None, 0.0, self.mode, _stream()), meta)
        _abi.check(code, 'um_linear_fwd')
        return out, m, n

    def linear_ln(self, a, weights, norm, residual=None, a_planes_k=None):
        """``LayerNorm(A . W^T) (+ residual)`` -> fp32 ``[M, 128]``; ``norm`` is an ``nn.LayerNorm`` over 128."""
        wp, n, k = self.weight_planes(weights)
        if a_planes_k is not None:
            m = a.numel() // (2 * self.nplanes * a_planes_k)
            args = (None, None, _ptr(a))
        else:
            m = a.shape[0]
            self._check_rows('a', a, k)
            args = (_ptr(a), None, None)
        if residual is not None:
            self._check_rows('residual', residual, n)
        out = torch.empty((m, n), dtype=torch.float32, device=a.device)
        code = self._launch('linear', lambda: self.lib.um_linear_fwd(
            args[0], args[1], args[2], _ptr(wp), m, n, k, self.WSHIFT, 1, _ptr(out),
            _ptr(norm.weight), _ptr(norm.bias), _ptr(residual) if residual is not None else None,
            float(norm.eps), self.mode, _stream()), {'flops': 2.0 * m * n * k})
        _abi.check(code, 'um_linear_fwd')
        return out

    def ffn_ln(self, x, y, w1, w2, norm, planes=False):
        """``x + LayerNorm(W2 . gelu(W1 . [x | y]))`` in one kernel (``um_ffn_fwd``); x, y fp32 ``[M, 128]``,
        ``w1`` ``[hidden, 256]``, ``w2`` ``[128, hidden]``, ``norm`` an ``nn.LayerNorm`` over 128.  ``planes``: the same launch also
        writes the result's operand planes ``[NS][M][128]`` (``um_ffn_planes_fwd``; bit for bit ``linear_planes(out, ())``) -> ``(out,
        planes)``: the next block's keys / values when the k | v projections are folded away."""
        w1p, hid, k1 = self.weight_planes((w1,))
        w2p, n2, k2 = self.weight_planes((w2,))
        if (k1, n2, k2) != (256, 128, hid):
            raise ValueError(f'ffn_ln: expected W1 [hidden, 256] and W2 [128, hidden], got {tuple(w1.shape)} {tuple(w2.shape)}')
        self._check_rows('x', x, 128)
        self._check_rows('y', y, 128)
        m = x.shape[0]
        if y.shape[0] != m:
            raise ValueError('ffn_ln: x and y must have the same number of rows')
        out = torch.empty((m, 128), dtype=torch.float32, device=x.device)
        ws = self._split_workspace('ffn_hsplit', (m, hid), x.device)
        if planes:
            pl = torch.empty(self.lib.um_planes_bytes(m, 128, self.mode), dtype=torch.uint8, device=x.device)
            code = self._launch('ffn', lambda: self.lib.um_ffn_planes_fwd(
                _ptr(x), _ptr(y), _ptr(w1p), _ptr(w2p), m, hid, self.WSHIFT, _ptr(norm.weight), _ptr(norm.bias),
                float(norm.eps), _ptr(out), _ptr(pl), self.mode, _ptr(ws) if ws is not None else None,
                ws.numel() if ws is not None else 0, _stream()), {'flops': 2.0 * m * hid * (256 + 128)})
            _abi.check(code, 'um_ffn_planes_fwd')
            return out, pl
        code = self._launch('ffn', lambda: self.lib.um_ffn_ws_fwd(
            _ptr(x), _ptr(y), _ptr(w1p), _ptr(w2p), m, hid, self.WSHIFT, _ptr(norm.weight), _ptr(norm.bias),
            float(norm.eps), _ptr(out), self.mode, _ptr(ws) if ws is not None else None, ws.numel() if ws is not None else 0,
            _stream()), {'flops': 2.0 * m * hid * (256 + 128)})
        _abi.check(code, 'um_ffn_ws_fwd')
        return out

    def ffn_ln_kv(self, x, y, w1, w2, norm, kv_weights):
        """:meth:`ffn_ln` plus the NEXT block's key / value projections of its result (:meth:`kv4_planes` of the returned tokens with
        ``kv_weights`` = next block's (k_self, v_self, k_cross, v_cross)) from the same launch (``um_ffn_kv_fwd``; small launches
        run the two kernels back to back inside the call) -> ``(out fp32 [M, 128], blocked k | v planes)``."""
        w1p, hid, k1 = self.weight_planes((w1,))
        w2p, n2, k2 = self.weight_planes((w2,))
        if (k1, n2, k2) != (256, 128, hid):
            raise ValueError(f'ffn_ln_kv: expected W1 [hidden, 256] and W2 [128, hidden], got {tuple(w1.shape)} {tuple(w2.shape)}')
        self._check_rows('x', x, 128)
        self._check_rows('y', y, 128)
        m = x.shape[0]
        if y.shape[0] != m:
            raise ValueError('ffn_ln_kv: x and y must have the same number of rows')
        wc = self.kv4_weight_planes(kv_weights)
        out = torch.empty((m, 128), dtype=torch.float32, device=x.device)
        kv = torch.empty(self.lib.um_planes_bytes(4 * m, 128, self.mode), dtype=torch.uint8, device=x.device)
        ws = self._split_workspace('ffn_hsplit', (m, hid), x.device)
        code = self._launch('ffn', lambda: self.lib.um_ffn_kv_fwd(
            _ptr(x), _ptr(y), _ptr(w1p), _ptr(w2p), m, hid, self.WSHIFT, _ptr(norm.weight), _ptr(norm.bias),
            float(norm.eps), _ptr(out), _ptr(wc), _ptr(kv), self.mode, _ptr(ws) if ws is not None else None,
            ws.numel() if ws is not None else 0, _stream()), {'flops': 2.0 * m * hid * (256 + 128) + 2.0 * m * 512 * 128})
        _abi.check(code, 'um_ffn_kv_fwd')
        return out, kv

    def window_attention_planes(self, q, k, v, streams, h, w, win_h, win_w, shift_h=0, shift_w=0, kv_rotate=0):
        """Attention on operand planes.  q, k, v: ``(plane_tensor, rows, cols, col_offset)`` -- a 128-column slice
        starting at ``col_offset`` of a ``[NS][rows][cols]`` plane tensor (k and v must share their tensor's shape)."""
        (qt, qrows, qcols, qoff), (kt, krows, kcols, koff), (vt, vrows, vcols, voff) = q, k, v
        if (krows, kcols) != (vrows, vcols) or qrows != streams * h * w or krows != qrows:
            raise ValueError('inconsistent plane shapes')
        out = torch.empty((streams, h * w, 128), dtype=torch.float32, device=qt.device)
        n = win_h * win_w
        meta = {'flops': 4.0 * streams * h * w * n * 128}
        code = self._launch('window_attn', lambda: self.lib.um_window_attn_planes_fwd(
            _ptr(qt) + 2 * qoff, _ptr(kt) + 2 * koff, _ptr(vt) + 2 * voff, _ptr(out), streams, h, w, 128,
            qcols, kcols, qrows * qcols, krows * kcols, win_h, win_w, shift_h, shift_w, kv_rotate, self.mode, _stream()), meta)
        _abi.check(code, 'um_window_attn_planes_fwd')
        return out

    def window_attention_merge(self, q, k, v, streams, h, w, win_h, win_w, shift_h, shift_w, kv_rotate, merge_weight, norm,
                               residual=None):
        """Attention on operand planes with ``LayerNorm(message . Wm^T) (+ residual)`` folded into the kernel's epilogue
        (``um_window_attn_merge_fwd``); arguments as :meth:`window_attention_planes`."""
        (qt, qrows, qcols, qoff), (kt, krows, kcols, koff), (vt, vrows, vcols, voff) = q, k, v
        if (krows, kcols) != (vrows, vcols) or qrows != streams * h * w or krows != qrows:
            raise ValueError('inconsistent plane shapes')
        wp, n, kk = self.weight_planes((merge_weight,))
        if (n, kk) != (128, 128):
            raise ValueError('window_attention_merge: the merge weight must be [128, 128]')
        if residual is not None:
            self._check_rows('residual', residual, 128)
        out = torch.empty((streams, h * w, 128), dtype=torch.float32, device=qt.device)
        meta = {'flops': 4.0 * streams * h * w * win_h * win_w * 128}
        code = self._launch('window_attn', lambda: self.lib.um_window_attn_merge_fwd(
            _ptr(qt) + 2 * qoff, _ptr(kt) + 2 * koff, _ptr(vt) + 2 * voff, _ptr(wp), _ptr(norm.weight), _ptr(norm.bias),
            _ptr(residual) if residual is not None else None, float(norm.eps), self.WSHIFT, _ptr(out), streams, h, w, 128,
            qcols, kcols, qrows * qcols, krows * kcols, win_h, win_w, shift_h, shift_w, kv_rotate, self.mode, _stream()), meta)
        _abi.check(code, 'um_window_attn_merge_fwd')
        return out

    def _split_workspace(self, kind, geometry, device):
        """Scratch of a split small launch, ``None`` when the launch is not split.  One buffer per geometry: the arrival counters sit
        at its head, one per tile, where a buffer of another geometry holds partial results."""
        size = self.lib.um_window_attn_ksplit_workspace_bytes if kind == 'attn_ksplit' else self.lib.um_ffn_split_workspace_bytes
        nbytes = size(*geometry)
        return self._workspace(kind, geometry, nbytes, device, self.GEOMETRIES) if nbytes else None

    def window_attention_qproj_merge(self, x, q_weight, k, v, streams, h, w, win_h, win_w, shift_h, shift_w, kv_rotate,
                                     merge_weight, norm, residual=None, fold=None):
        """:meth:`window_attention_merge` with ``q = x . Wq^T`` computed in the kernel's prologue
        (``um_window_attn_qproj_merge_fwd``): ``x`` fp32 ``[streams*h*w, 128]`` source tokens, ``q_weight`` ``[128, 128]``.
        ``fold = (k_weight, v_weight)``: ``k`` and ``v`` are the planes of the UNPROJECTED key / value tokens and the kernel runs with
        the folded weights ``Wk^T Wq`` and ``Wm Wv`` (:func:`fold_weights`) -- the same logits and messages with no k | v projection."""
        # k, v: (plane tensor, rows, row stride in elements, element offset of the first row[, plane stride in elements]) -- the
        # optional fifth entry describes slices of a bigger plane tensor (the blocked [NS][4][M][128] k | v planes of kv4_planes)
        (kt, krows, kcols, koff), (vt, vrows, vcols, voff) = k[:4], v[:4]
        kps = k[4] if len(k) > 4 else krows * kcols
        if (v[4] if len(v) > 4 else vrows * vcols) != kps:
            raise ValueError('k and v must share their plane stride')
        self._check_rows('x', x, 128)
        if (krows, kcols) != (vrows, vcols) or x.shape[0] != streams * h * w or krows != x.shape[0]:
            raise ValueError('inconsistent plane shapes')
        if fold is not None:
            q_weight, merge_weight = self._folded_weight('q', fold[0], q_weight), self._folded_weight('m', merge_weight, fold[1])
        wqp, nq, kq = self.weight_planes((q_weight,))
        wp, n, kk = self.weight_planes((merge_weight,))
        if (n, kk, nq, kq) != (128, 128, 128, 128):
            raise ValueError('window_attention_qproj_merge: the query and merge weights must be [128, 128]')
        if residual is not None:
            self._check_rows('residual', residual, 128)
        out = torch.empty((streams, h * w, 128), dtype=torch.float32, device=x.device)
        meta = {'flops': 4.0 * streams * h * w * win_h * win_w * 128}
        ks = self._split_workspace('attn_ksplit', (streams, h, w, win_h, win_w), x.device)
        code = self._launch('window_attn', lambda: self.lib.um_window_attn_qproj_merge_fwd(
            _ptr(x), _ptr(wqp), _ptr(kt) + 2 * koff, _ptr(vt) + 2 * voff, _ptr(wp), _ptr(norm.weight), _ptr(norm.bias),
            _ptr(residual) if residual is not None else None, float(norm.eps), self.WSHIFT, _ptr(out), streams, h, w, 128,
            kcols, kps, win_h, win_w, shift_h, shift_w, kv_rotate, self.mode,
            _ptr(ks) if ks is not None else None, ks.numel() if ks is not None else 0, _stream()), meta)
        _abi.check(code, 'um_window_attn_qproj_merge_fwd')
        return out

    # ------------------------------------------------------------------ k | v projections of a whole Transformer block
    def kv4_weight_planes(self, weights):
        """Planes of the packed ``[256, 256]`` weight of ``um_kv4_fwd`` / ``um_ffn_kv_fwd`` from the four ``[128, 128]`` projection
        weights (k_self, v_self, k_cross, v_cross): ``Wc[32c + r, :128] = W4[32c + r]``, ``Wc[32c + r, 128:] = W4[256 + 32c + (r ^ 16)]``
        (include/unimatch_hip.h, um_kv4_fwd); cached until a weight changes."""
        key, hit = self._cache_get('kv4', weights)
        if hit is not None:
            return hit
        if len(weights) != 4 or any(tuple(w.shape) != (128, 128) for w in weights):
            raise ValueError('kv4_weight_planes: expected four [128, 128] weights (k_self, v_self, k_cross, v_cross)')
        wc = pack_kv4_weights(weights)                                               # [256, 256]
        self._check_weight_range(wc, self.WSHIFT if self.mode == 0 else 0, 'Linear weight')
        planes = torch.empty(self.lib.um_planes_bytes(256, 256, self.mode), dtype=torch.uint8, device=wc.device)
        _abi.check(self.lib.um_weight_planes(_ptr(wc), _ptr(planes), 256, 256, self.WSHIFT, self.mode, _stream()), 'um_weight_planes')
        return self._cache_put(key, weights, planes)

    @staticmethod
    def kv4_slices(kv, m):
        """The four projections of blocked k | v planes ``[NS][4][m][128]`` as attention operands: ``((k_self, v_self), (k_cross, v_cross))``."""
        part = lambda j: (kv, m, 128, j * m * 128, 4 * m * 128)
        return (part(0), part(1)), (part(2), part(3))

    def kv4_planes(self, x, weights):
        """``um_kv4_fwd``: both layers' key / value projections of a Transformer block (four bias-free 128 x 128 Linears of the
        token stream ``x`` fp32 ``[M, 128]``, transformer.py:58-60) in one launch -> blocked operand planes ``[NS][4][M][128]``."""
        self._check_rows('x', x, 128)
        wc = self.kv4_weight_planes(weights)
        m = x.shape[0]
        out = torch.empty(self.lib.um_planes_bytes(4 * m, 128, self.mode), dtype=torch.uint8, device=x.device)
        code = self._launch('linear', lambda: self.lib.um_kv4_fwd(_ptr(x), _ptr(wc), m, self.WSHIFT, _ptr(out), self.mode, _stream()),
                            {'flops': 2.0 * m * 512 * 128})
        _abi.check(code, 'um_kv4_fwd')
        return out

    # ------------------------------------------------------------------ convex upsampling (SURVEY 8(f) "next" row)
    def convex_upsample(self, flow, mask, factor, is_depth=False, mask_nhwc=False, out=None):
        """RAFT convex upsampling of ``flow [B,V,h,w]`` with ``mask [B,9*factor^2,h,w]`` (or NHWC ``[B*h*w, 9*factor^2]``
        with ``mask_nhwc``) -> ``[B,V,factor*h,factor*w]``.  ``out``: the destination, a contiguous fp32 tensor of that shape on the
        flow's device (a batch slice of a bigger prediction); it is what the call returns."""
        b, v, h, w = flow.shape
        want = (b * h * w, 9 * factor * factor) if mask_nhwc else (b, 9 * factor * factor, h, w)
        if not (flow.is_cuda and flow.dtype == torch.float32 and mask.dtype == torch.float32 and tuple(mask.shape) == want):
            raise ValueError(f'convex_upsample: bad shapes flow {tuple(flow.shape)} mask {tuple(mask.shape)}')
        flow, mask = flow.contiguous(), mask.contiguous()
        up = out
        if up is None:
            up = torch.empty((b, v, factor * h, factor * w), dtype=torch.float32, device=flow.device)
        elif not (tuple(up.shape) == (b, v, factor * h, factor * w) and up.dtype == torch.float32 and up.device == flow.device
                  and up.is_contiguous()):
            raise ValueError(f'convex_upsample: out must be a contiguous float32 [{b}, {v}, {factor * h}, {factor * w}] tensor on '
                             f'{flow.device}, got {tuple(up.shape)} {up.dtype} {up.device}')
        code = self._launch('convex_upsample', lambda: self.lib.um_convex_upsample(
            _ptr(flow), _ptr(mask), _ptr(up), b, v, h, w, factor, int(bool(is_depth)), int(bool(mask_nhwc)), _stream()))
        _abi.check(code, 'um_convex_upsample')
        return up

    def flow_warp(self, tokens, flow, h, w):
        """``um_flow_warp``: bilinear warp of token-major features ``[b, h*w, c]`` by ``flow [b,2,h,w]`` -> tokens."""
        b, l, c = tokens.shape
        if not (tokens.is_cuda and tokens.dtype == torch.float32 and tokens.is_contiguous() and l == h * w
                and tuple(flow.shape) == (b, 2, h, w) and flow.dtype == torch.float32):
            raise ValueError(f'flow_warp: bad shapes tokens {tuple(tokens.shape)} flow {tuple(flow.shape)}')
        flow = flow.contiguous()
        out = torch.empty_like(tokens)
        code = self._launch('convex_upsample', lambda: self.lib.um_flow_warp(
            _ptr(tokens), _ptr(flow), _ptr(out), b, h, w, c, _stream()))
        _abi.check(code, 'um_flow_warp')
        return out

    def fwd_bwd_occlusion(self, fwd, bwd, alpha=0.01, beta=0.5):
        """``um_fwd_bwd_occlusion``: forward / backward occlusion masks ``[B, H, W]`` fp32 in {0, 1} of the flows ``fwd``, ``bwd``
        ``[B, 2, H, W]`` (the reference's forward_backward_consistency_check in one launch)."""
        if not (fwd.is_cuda and fwd.dtype == torch.float32 and fwd.dim() == 4 and fwd.shape[1] == 2
                and bwd.shape == fwd.shape and bwd.dtype == torch.float32 and bwd.device == fwd.device):
            raise ValueError(f'fwd_bwd_occlusion: expected two CUDA float32 [B, 2, H, W] flows of one shape, got '
                             f'{tuple(fwd.shape)} {fwd.dtype} and {tuple(bwd.shape)} {bwd.dtype}')
        fwd, bwd = fwd.contiguous(), bwd.contiguous()
        b, _, h, w = fwd.shape
        occ_f = torch.empty((b, h, w), dtype=torch.float32, device=fwd.device)
        occ_b = torch.empty_like(occ_f)
        code = self._launch('fwd_bwd_occlusion', lambda: self.lib.um_fwd_bwd_occlusion(
            _ptr(fwd), _ptr(bwd), _ptr(occ_f), _ptr(occ_b), b, h, w, float(alpha), float(beta), _stream()))
        _abi.check(code, 'um_fwd_bwd_occlusion')
        return occ_f, occ_b

    def flow_to_rgb(self, flow):
        """``um_flow_to_rgb``: Middlebury colouring ``[B, H, W, 3]`` uint8 of ``flow [B, 2, H, W]``, each image normalised by its own
        maximum (the reference's flow_to_image per image)."""
        if not (flow.is_cuda and flow.dtype == torch.float32 and flow.dim() == 4 and flow.shape[1] == 2):
            raise ValueError(f'flow_to_rgb: expected a CUDA float32 [B, 2, H, W] flow, got {tuple(flow.shape)} {flow.dtype}')
        flow = flow.contiguous()
        b, _, h, w = flow.shape
        rgb = torch.empty((b, h, w, 3), dtype=torch.uint8, device=flow.device)
        ws = self._ws(self.lib.um_flow_to_rgb_workspace_bytes(b, h, w), flow.device)
        code = self._launch('flow_to_rgb', lambda: self.lib.um_flow_to_rgb(
            _ptr(flow), _ptr(rgb), b, h, w, _ptr(ws), ws.numel(), _stream()))
        _abi.check(code, 'um_flow_to_rgb')
        return rgb

    def flow_chain(self, flow, occ=None, points=None, alive=None, stride=1):
        """``um_flow_chain``: follow points through the flows ``flow [P, 2, H, W]`` of consecutive pairs in one launch ->
        ``(tracks [P, N, 2] float32, visible [P, N] bool)``.  ``occ [P, H, W]`` (1 = occluded) ends a track whose sample of it reaches
        0.5; ``points [N, 2]`` as (x, y) (``None``: every ``stride``-th pixel of every ``stride``-th row) and ``alive [N]`` bool are
        the start -- the last rows of an earlier call continue it."""
        if not (flow.is_cuda and flow.dtype == torch.float32 and flow.dim() == 4 and flow.shape[1] == 2):
            raise ValueError(f'flow_chain: flow: expected a CUDA float32 [P, 2, H, W] tensor, got {tuple(flow.shape)} {flow.dtype}')
        p, _, h, w = flow.shape
        if occ is not None and not (occ.dtype == torch.float32 and occ.device == flow.device and tuple(occ.shape) == (p, h, w)):
            raise ValueError(f'flow_chain: occ: expected float32 {(p, h, w)} on {flow.device}, got {tuple(occ.shape)} {occ.dtype} '
                             f'on {occ.device}')
        if points is not None:
            if not (points.dtype == torch.float32 and points.device == flow.device and points.dim() == 2 and points.shape[1] == 2):
                raise ValueError(f'flow_chain: points: expected float32 [N, 2] on {flow.device}, got {tuple(points.shape)} '
                                 f'{points.dtype} on {points.device}')
            n = points.shape[0]
            points = points.contiguous()
        else:
            if int(stride) < 1:
                raise ValueError(f'flow_chain: stride must be >= 1, got {stride}')
            n = -(-h // int(stride)) * -(-w // int(stride))
        if alive is not None:
            if not (alive.dtype == torch.bool and alive.device == flow.device and tuple(alive.shape) == (n,)):
                raise ValueError(f'flow_chain: alive: expected bool {(n,)} on {flow.device}, got {tuple(alive.shape)} {alive.dtype} '
                                 f'on {alive.device}')
            alive = alive.contiguous().view(torch.uint8)
        flow = flow.contiguous()
        occ = None if occ is None else occ.contiguous()
        tracks = torch.empty((p, n, 2), dtype=torch.float32, device=flow.device)
        visible = torch.empty((p, n), dtype=torch.uint8, device=flow.device)
        opt = lambda t: None if t is None else _ptr(t)
        code = self._launch('flow_chain', lambda: self.lib.um_flow_chain(
            _ptr(flow), opt(occ), opt(points), opt(alive), _ptr(tracks), _ptr(visible), p, h, w, n, int(stride), _stream()),
            {'bytes': 21.0 * p * n})
        _abi.check(code, 'um_flow_chain')
        return tracks, visible.view(torch.bool)

    # ------------------------------------------------------------------ inference-size handling
    @staticmethod
    def _check_sizing(name, mode, size, crop):
        if mode not in ('pad', 'resize'):
            raise ValueError(f"{name}: mode must be 'pad' or 'resize', got {mode!r}")
        (hp, wp), (top, left) = (int(s) for s in size), (int(c) for c in crop)
        if hp < 1 or wp < 1:
            raise ValueError(f'{name}: the inference size {hp}x{wp} is empty')
        return (1 if mode == 'resize' else 0), hp, wp, top, left

    def image_prepare(self, images, size, mode='pad', crop=(0, 0), transpose=False, mean=None, std=None, hflip=False, out=None):
        """``um_image_prepare``: ``images`` -- fp32 ``[B, 3, H, W]`` or uint8 ``[B, H, W, 3]`` -- to the model's input ``[B, 3, hp,
        wp]`` fp32 with ``size = (hp, wp)``: optional transpose, ``(x / 255 - mean) / std`` when ``mean`` / ``std`` (three floats each)
        are given, then ``mode='pad'`` (replicate padding, the image at ``crop = (top, left)``) or ``'resize'`` (bilinear,
        align_corners), then ``hflip``: a mirror of x inside the same launch (``um_image_prepare_flip``), bit for bit ``torch.flip`` of the
        unflipped result.  ``out``: a preallocated contiguous fp32 ``[B, 3, hp, wp]`` tensor (a batch slice of a larger one) to write
        into.  Enqueued on the current stream: no synchronisation, no copy."""
        u8 = images.dtype == torch.uint8
        ok = images.is_cuda and images.dim() == 4 and (u8 or images.dtype == torch.float32) and images.shape[3 if u8 else 1] == 3
        if not ok:
            raise ValueError(f'image_prepare: expected a CUDA float32 [B, 3, H, W] or uint8 [B, H, W, 3] tensor, got '
                             f'{tuple(images.shape)} {images.dtype} {images.device}')
        if (mean is None) != (std is None) or (mean is not None and (len(mean) != 3 or len(std) != 3)):
            raise ValueError('image_prepare: mean and std are three floats each, given together')
        m, hp, wp, top, left = self._check_sizing('image_prepare', mode, size, crop)
        images = images.contiguous()
        b = images.shape[0]
        h, w = (images.shape[1:3] if u8 else images.shape[2:])
        ih, iw = (w, h) if transpose else (h, w)
        if m == 0 and (top < 0 or left < 0 or top + ih > hp or left + iw > wp):
            raise ValueError(f'image_prepare: the image {ih}x{iw} at ({top}, {left}) leaves the padded size {hp}x{wp}')
        if out is None:
            out = torch.empty((b, 3, hp, wp), dtype=torch.float32, device=images.device)
        elif not (out.is_cuda and out.device == images.device and out.dtype == torch.float32 and tuple(out.shape) == (b, 3, hp, wp)
                  and out.is_contiguous()):
            raise ValueError(f'image_prepare: out must be a contiguous CUDA float32 [{b}, 3, {hp}, {wp}] tensor on {images.device}, got '
                             f'{tuple(out.shape)} {out.dtype} {out.device}')
        fmean = (ctypes.c_float * 3)(*mean) if mean is not None else None
        fstd = (ctypes.c_float * 3)(*std) if std is not None else None
        code = self._launch('image_prepare', lambda: self.lib.um_image_prepare_flip(
            _ptr(images), 1 if u8 else 0, _ptr(out), b, h, w, int(bool(transpose)), fmean, fstd, m, hp, wp, top, left, int(bool(hflip)),
            _stream()))
        _abi.check(code, 'um_image_prepare_flip')
        return out

    def pred_restore(self, pred, size, mode='pad', crop=(0, 0), kind='flow', transpose=False, hflip=False, out=None):
        """``um_pred_restore``: the prediction ``pred [B, C, hp, wp]`` back to the caller's frame ``size = (H, W)``: ``mode='pad'``
        crops at ``crop = (top, left)``, ``'resize'`` resizes and rescales by ``kind`` (``'flow'``: ``u * W / wp``, ``v * H / hp``;
        ``'disparity'``: ``* W / wp``; ``'depth'``: nothing), then the optional transpose back (flow channels are not swapped), then
        ``hflip``: a mirror of x inside the same launch (``um_pred_restore_flip``).  ``out``: a preallocated contiguous fp32
        ``[B, C, H, W]`` tensor to write into."""
        kinds = {'flow': 0, 'disparity': 1, 'depth': 2}
        if kind not in kinds:
            raise ValueError(f'pred_restore: kind must be one of {sorted(kinds)}, got {kind!r}')
        if not (pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 4 and pred.shape[1] == (2 if kind == 'flow' else 1)):
            raise ValueError(f"pred_restore: expected a CUDA float32 [B, {2 if kind == 'flow' else 1}, hp, wp] {kind}, got "
                             f'{tuple(pred.shape)} {pred.dtype} {pred.device}')
        m, h, w, top, left = self._check_sizing('pred_restore', mode, size, crop)
        pred = pred.contiguous()
        b, c, hp, wp = pred.shape
        ih, iw = (w, h) if transpose else (h, w)
        if m == 0 and (top < 0 or left < 0 or top + ih > hp or left + iw > wp):
            raise ValueError(f'pred_restore: the crop {ih}x{iw} at ({top}, {left}) leaves the prediction {hp}x{wp}')
        if out is None:
            out = torch.empty((b, c, h, w), dtype=torch.float32, device=pred.device)
        elif not (out.is_cuda and out.device == pred.device and out.dtype == torch.float32 and tuple(out.shape) == (b, c, h, w)
                  and out.is_contiguous()):
            raise ValueError(f'pred_restore: out must be a contiguous CUDA float32 [{b}, {c}, {h}, {w}] tensor on {pred.device}, got '
                             f'{tuple(out.shape)} {out.dtype} {out.device}')
        code = self._launch('pred_restore', lambda: self.lib.um_pred_restore_flip(
            _ptr(pred), _ptr(out), b, c, hp, wp, m, top, left, h, w, kinds[kind], int(bool(transpose)), int(bool(hflip)), _stream()))
        _abi.check(code, 'um_pred_restore_flip')
        return out

    # ------------------------------------------------------------------ colour maps of scalar predictions
    NORMS = {'minmax_255': 0, 'min_p95_256': 1}

    def scalar_to_rgb(self, x, lut, inverse=False, norm='minmax_255', return_stats=False):
        """``um_scalar_to_rgb``: ``x [B, H, W]`` fp32 -> ``[B, H, W, 3]`` uint8 through the device table ``lut [256, 3]`` uint8, each
        image normalised on its own: ``norm='minmax_255'`` between its minimum and maximum (the reference's vis_disparity),
        ``'min_p95_256'`` between its minimum and its 95th percentile (viz_depth_tensor); ``inverse``: of ``1 / x``.
        ``return_stats``: also ``[B, 2]`` fp32 ``(vmin, vmax)``.  Enqueued on the current stream: no synchronisation, no copy."""
        if norm not in self.NORMS:
            raise ValueError(f'scalar_to_rgb: norm must be one of {sorted(self.NORMS)}, got {norm!r}')
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3):
            raise ValueError(f'scalar_to_rgb: expected a CUDA float32 [B, H, W] tensor, got {tuple(x.shape)} {x.dtype} {x.device}')
        if not (lut.is_cuda and lut.device == x.device and lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3) and lut.is_contiguous()):
            raise ValueError(f'scalar_to_rgb: expected a contiguous uint8 [256, 3] table on {x.device}, got {tuple(lut.shape)} {lut.dtype} '
                             f'{lut.device}')
        x = x.contiguous()
        b, h, w = x.shape
        rgb = torch.empty((b, h, w, 3), dtype=torch.uint8, device=x.device)
        stats = torch.empty((b, 2), dtype=torch.float32, device=x.device) if return_stats else None
        ws = self._ws(self.lib.um_scalar_to_rgb_workspace_bytes(b, h, w), x.device)
        code = self._launch('scalar_to_rgb', lambda: self.lib.um_scalar_to_rgb(
            _ptr(x), _ptr(rgb), b, h, w, int(bool(inverse)), self.NORMS[norm], _ptr(lut), _ptr(stats) if return_stats else None,
            _ptr(ws), ws.numel(), _stream()))
        _abi.check(code, 'um_scalar_to_rgb')
        return (rgb, stats) if return_stats else rgb

    # ------------------------------------------------------------------ evaluation metrics
    @staticmethod
    def _metric_args(name, pred, gt, channels, crop, masks):
        """Shape / dtype checks shared by the three metric wrappers: ``pred`` still padded, ``gt`` and the masks at the crop's size.
        Returns the contiguous tensors and ``(b, hp, wp, h, w, top, left)``."""
        want = 4 if channels else 3
        ok = (pred.is_cuda and pred.dtype == torch.float32 and gt.dtype == torch.float32 and gt.device == pred.device
              and pred.dim() == want and gt.dim() == want and gt.shape[0] == pred.shape[0]
              and (not channels or (pred.shape[1] == channels and gt.shape[1] == channels)))
        if not ok:
            raise ValueError(f'{name}: expected CUDA float32 pred / gt of {want} dimensions and one batch, got {tuple(pred.shape)} '
                             f'{pred.dtype} and {tuple(gt.shape)} {gt.dtype}')
        b, (hp, wp), (h, w) = pred.shape[0], pred.shape[-2:], gt.shape[-2:]
        top, left = (int(crop[0]), int(crop[1])) if crop is not None else (0, 0)
        if top < 0 or left < 0 or top + h > hp or left + w > wp:
            raise ValueError(f'{name}: the crop {h}x{w} at ({top}, {left}) leaves the prediction {hp}x{wp}')
        out = []
        for m in masks:
            if m is not None:
                if not (m.is_cuda and m.device == pred.device and tuple(m.shape) == (b, h, w)):
                    raise ValueError(f'{name}: expected a CUDA mask [{b}, {h}, {w}], got {tuple(m.shape)} on {m.device}')
                m = m.float().contiguous()
            out.append(m)
        return pred.contiguous(), gt.contiguous(), out, (b, hp, wp, h, w, top, left)

    def flow_metrics(self, pred, gt, valid=None, noc_valid=None, crop=None):
        """``um_flow_metrics``: one row ``[16]`` float64 of end-point-error accumulators per sample (layout in the header) of the
        padded prediction ``pred [B, 2, Hp, Wp]`` against ``gt [B, 2, H, W]`` at the crop offset ``crop = (top, left)``; ``valid``,
        ``noc_valid`` ``[B, H, W]`` or None.  Enqueued on the current stream: no synchronisation, no copy."""
        pred, gt, (valid, noc_valid), (b, hp, wp, h, w, top, left) = self._metric_args('flow_metrics', pred, gt, 2, crop, (valid, noc_valid))
        rows = torch.empty((b, 16), dtype=torch.float64, device=pred.device)
        ws = self._ws(self.lib.um_flow_metrics_workspace_bytes(b, h, w), pred.device)
        code = self._launch('flow_metrics', lambda: self.lib.um_flow_metrics(
            _ptr(pred), _ptr(gt), _ptr(valid) if valid is not None else None, _ptr(noc_valid) if noc_valid is not None else None,
            _ptr(rows), b, hp, wp, h, w, top, left, _ptr(ws), ws.numel(), _stream()))
        _abi.check(code, 'um_flow_metrics')
        return rows

    def disp_metrics(self, pred, gt, max_disp=0.0, crop=None):
        """``um_disp_metrics``: one row ``[8]`` float64 per sample of ``pred [B, Hp, Wp]`` against ``gt [B, H, W]`` over ``gt > 0``
        (and ``gt < max_disp`` when ``max_disp > 0``)."""
        pred, gt, _, (b, hp, wp, h, w, top, left) = self._metric_args('disp_metrics', pred, gt, 0, crop, ())
        rows = torch.empty((b, 8), dtype=torch.float64, device=pred.device)
        ws = self._ws(self.lib.um_disp_metrics_workspace_bytes(b, h, w), pred.device)
        code = self._launch('disp_metrics', lambda: self.lib.um_disp_metrics(
            _ptr(pred), _ptr(gt), _ptr(rows), b, hp, wp, h, w, top, left, float(max_disp), _ptr(ws), ws.numel(), _stream()))
        _abi.check(code, 'um_disp_metrics')
        return rows

    def depth_metrics(self, pred, gt, valid=None, lo=0.0, hi=float('inf'), crop=None):
        """``um_depth_metrics``: one row ``[8]`` float64 per sample of ``pred [B, Hp, Wp]`` against ``gt [B, H, W]`` over
        ``lo < gt < hi`` and ``valid > 0.5``."""
        pred, gt, (valid,), (b, hp, wp, h, w, top, left) = self._metric_args('depth_metrics', pred, gt, 0, crop, (valid,))
        rows = torch.empty((b, 8), dtype=torch.float64, device=pred.device)
        ws = self._ws(self.lib.um_depth_metrics_workspace_bytes(b, h, w), pred.device)
        code = self._launch('depth_metrics', lambda: self.lib.um_depth_metrics(
            _ptr(pred), _ptr(gt), _ptr(valid) if valid is not None else None, _ptr(rows), b, hp, wp, h, w, top, left, float(lo),
            float(hi), _ptr(ws), ws.numel(), _stream()))
        _abi.check(code, 'um_depth_metrics')
        return rows

    def flow_upsample2x(self, flow, mult=2.0):
        """``mult * F.interpolate(flow, scale_factor=2, mode='bilinear', align_corners=True)`` (``um_flow_upsample2x``)."""
        if not (flow.is_cuda and flow.dtype == torch.float32 and flow.dim() == 4):
            raise ValueError('flow_upsample2x: expected a CUDA float32 [B, V, h, w] tensor')
        flow = flow.contiguous()
        b, v, h, w = flow.shape
        out = torch.empty((b, v, 2 * h, 2 * w), dtype=torch.float32, device=flow.device)
        _abi.check(self.lib.um_flow_upsample2x(_ptr(flow), _ptr(out), b, v, h, w, float(mult), _stream()), 'um_flow_upsample2x')
        return out

    def depth_cam(self, intrinsics, pose, stride_div, bidir=False):
        """``[B or 2B, 30]`` = K^-1 | R | t | K of the depth kernels from the caller's intrinsics ``[B,3,3]`` (rows 0-1 divided by
        ``stride_div``) and pose ``[B,4,4]`` (``um_depth_cam_pack``; with ``bidir`` the second half carries the inverse pose)."""
        b = intrinsics.shape[0]
        if not (tuple(intrinsics.shape) == (b, 3, 3) and tuple(pose.shape) == (b, 4, 4) and intrinsics.is_cuda and pose.is_cuda):
            raise ValueError('depth_cam: expected CUDA intrinsics [B,3,3] and pose [B,4,4]')
        k, p = intrinsics.float().contiguous(), pose.float().contiguous()
        cam = torch.empty((2 * b if bidir else b, 30), dtype=torch.float32, device=k.device)
        _abi.check(self.lib.um_depth_cam_pack(_ptr(k), _ptr(p), _ptr(cam), b, float(stride_div), int(bool(bidir)), _stream()),
                   'um_depth_cam_pack')
        return cam

    def rigid_flow(self, inv_depth, cam):
        """Flow induced by inverse depth ``[B,1,h,w]`` and ``cam [B,30]`` (``um_rigid_flow``, geometry.py:99-195)."""
        b, _, h, w = inv_depth.shape
        if not (inv_depth.is_cuda and inv_depth.dtype == torch.float32 and tuple(cam.shape) == (b, 30)):
            raise ValueError('rigid_flow: expected CUDA float32 inv_depth [B,1,h,w] and cam [B,30]')
        inv_depth = inv_depth.contiguous()
        out = torch.empty((b, 2, h, w), dtype=torch.float32, device=inv_depth.device)
        _abi.check(self.lib.um_rigid_flow(_ptr(inv_depth), _ptr(cam), _ptr(out), b, h, w, _stream()), 'um_rigid_flow')
        return out

    def relative_pose_pairs(self, poses):
        """``[T-1, 4, 4]``: ``inv(poses[t+1]) @ poses[t]`` of the consecutive pairs of ``poses [T, 4, 4]`` (absolute camera-to-world,
        ``T >= 2``) on the current stream, no synchronisation (``um_relative_pose_pairs``)."""
        if not (poses.dim() == 3 and tuple(poses.shape[1:]) == (4, 4) and poses.shape[0] >= 2 and poses.is_cuda):
            raise ValueError('relative_pose_pairs: expected CUDA poses [T,4,4] with T >= 2')
        p = poses.float().contiguous()
        rel = torch.empty((p.shape[0] - 1, 4, 4), dtype=torch.float32, device=p.device)
        _abi.check(self.lib.um_relative_pose_pairs(_ptr(p), _ptr(rel), p.shape[0], _stream()), 'um_relative_pose_pairs')
        return rel

    # ------------------------------------------------------------------ cross-view consistency and point clouds (csrc/geometry.hip)
    def disp_consistency(self, disp_left, disp_right, alpha=0.01, beta=0.5):
        """``um_disp_consistency``: left / right occlusion masks ``[B, H, W]`` fp32 in {0, 1} of the disparities ``disp_left``,
        ``disp_right`` ``[B, H, W]`` (the flow check on ``(-disp_left, 0)`` / ``(disp_right, 0)``, one launch, two taps per pixel)."""
        dl, dr = disp_left, disp_right
        if not (dl.is_cuda and dl.dtype == torch.float32 and dl.dim() == 3 and dl.shape[-1] >= 2
                and dr.shape == dl.shape and dr.dtype == torch.float32 and dr.device == dl.device):
            raise ValueError(f'disp_consistency: expected two CUDA float32 [B, H, W >= 2] disparities of one shape, got '
                             f'{tuple(dl.shape)} {dl.dtype} and {tuple(dr.shape)} {dr.dtype}')
        dl, dr = dl.contiguous(), dr.contiguous()
        b, h, w = dl.shape
        occ_l = torch.empty((b, h, w), dtype=torch.float32, device=dl.device)
        occ_r = torch.empty_like(occ_l)
        code = self._launch('disp_consistency', lambda: self.lib.um_disp_consistency(
            _ptr(dl), _ptr(dr), _ptr(occ_l), _ptr(occ_r), b, h, w, float(alpha), float(beta), _stream()))
        _abi.check(code, 'um_disp_consistency')
        return occ_l, occ_r

    def depth_consistency(self, depth_ref, depth_src, cam_fwd, cam_inv, px_thr=1.0, rel_thr=0.01, return_errors=False):
        """``um_depth_consistency``: ``occ [B, H, W]`` fp32 in {0, 1} (and ``err_px``, ``err_rel`` with ``return_errors``) of the metric
        depths ``depth_ref``, ``depth_src`` ``[B, H, W]`` under the cam records ``cam_fwd``, ``cam_inv`` ``[B, 30]`` of the
        ref -> src pose and its inverse (the halves of ``depth_cam(..., 1, bidir=True)``)."""
        a, s = depth_ref, depth_src
        if not (a.is_cuda and a.dtype == torch.float32 and a.dim() == 3 and s.shape == a.shape and s.dtype == torch.float32
                and s.device == a.device):
            raise ValueError(f'depth_consistency: expected two CUDA float32 [B, H, W] depths of one shape, got '
                             f'{tuple(a.shape)} {a.dtype} and {tuple(s.shape)} {s.dtype}')
        b, h, w = a.shape
        for name, cam in (('cam_fwd', cam_fwd), ('cam_inv', cam_inv)):
            if not (cam.is_cuda and cam.dtype == torch.float32 and tuple(cam.shape) == (b, 30) and cam.device == a.device):
                raise ValueError(f'depth_consistency: expected {name} as CUDA float32 [{b}, 30], got {tuple(cam.shape)} {cam.dtype}')
        a, s, cam_fwd, cam_inv = a.contiguous(), s.contiguous(), cam_fwd.contiguous(), cam_inv.contiguous()
        occ = torch.empty((b, h, w), dtype=torch.float32, device=a.device)
        err_px = torch.empty_like(occ) if return_errors else None
        err_rel = torch.empty_like(occ) if return_errors else None
        code = self._launch('depth_consistency', lambda: self.lib.um_depth_consistency(
            _ptr(a), _ptr(s), _ptr(cam_fwd), _ptr(cam_inv), _ptr(occ), _ptr(err_px) if return_errors else None,
            _ptr(err_rel) if return_errors else None, b, h, w, float(px_thr), float(rel_thr), _stream()))
        _abi.check(code, 'um_depth_consistency')
        return (occ, err_px, err_rel) if return_errors else occ

    def points_pack(self, depth, cam_world, keep=None, colors=None, min_depth=0., max_depth=float('inf'), stride=1):
        """``um_points_pack``: ``(xyz [M, 3] fp32, rgb [M, 3] uint8 or None, count)`` -- the world points of the selected pixels of
        ``depth [B, H, W]`` under ``cam_world [B, 30]`` in ascending ``(b, y, x)`` order, in buffers of ``M`` = every candidate pixel;
        ``count`` is a one-element int32 tensor ON THE DEVICE holding N: rows ``N..M-1`` are unwritten.  No synchronisation here."""
        if not (depth.is_cuda and depth.dtype == torch.float32 and depth.dim() == 3):
            raise ValueError(f'points_pack: expected a CUDA float32 [B, H, W] depth, got {tuple(depth.shape)} {depth.dtype}')
        b, h, w = depth.shape
        stride = int(stride)
        if stride < 1:
            raise ValueError(f'points_pack: stride must be >= 1, got {stride}')
        if not (cam_world.is_cuda and cam_world.dtype == torch.float32 and tuple(cam_world.shape) == (b, 30)):
            raise ValueError(f'points_pack: expected cam_world as CUDA float32 [{b}, 30], got {tuple(cam_world.shape)} {cam_world.dtype}')
        if keep is not None and not (keep.is_cuda and keep.dtype == torch.float32 and keep.shape == depth.shape):
            raise ValueError(f'points_pack: expected keep as CUDA float32 {tuple(depth.shape)}, got {tuple(keep.shape)} {keep.dtype}')
        if colors is not None and not (colors.is_cuda and colors.dtype == torch.uint8 and tuple(colors.shape) == (b, h, w, 3)):
            raise ValueError(f'points_pack: expected colors as CUDA uint8 {(b, h, w, 3)}, got {tuple(colors.shape)} {colors.dtype}')
        depth, cam_world = depth.contiguous(), cam_world.contiguous()
        keep = None if keep is None else keep.contiguous()
        colors = None if colors is None else colors.contiguous()
        m = b * (-(-h // stride)) * (-(-w // stride))
        xyz = torch.empty((m, 3), dtype=torch.float32, device=depth.device)
        rgb = None if colors is None else torch.empty((m, 3), dtype=torch.uint8, device=depth.device)
        count = torch.empty(1, dtype=torch.int32, device=depth.device)
        ws = self._ws(self.lib.um_points_workspace_bytes(b, h, w, stride), depth.device)
        code = self._launch('points_pack', lambda: self.lib.um_points_pack(
            _ptr(depth), _ptr(cam_world), None if keep is None else _ptr(keep), None if colors is None else _ptr(colors), _ptr(xyz),
            None if rgb is None else _ptr(rgb), _ptr(count), b, h, w, stride, float(min_depth), float(max_depth), _ptr(ws), ws.numel(),
            _stream()))
        _abi.check(code, 'um_points_pack')
        return xyz, rgb, count

    # ------------------------------------------------------------------ encoder helper (outside the hot path)
    def instance_norm(self, x, relu=True, shortcut=None, eps=1e-5):
        """Fused InstanceNorm2d(affine=False) [+ ReLU] [+ shortcut, ReLU] on a contiguous NCHW fp32 map."""
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
            raise ValueError('instance_norm: expected a contiguous CUDA float32 NCHW tensor')
        if shortcut is not None and not (shortcut.shape == x.shape and shortcut.is_contiguous()
                                         and shortcut.dtype == torch.float32):
            raise ValueError('instance_norm: shortcut must match x')
        n, c, h, w = x.shape
        y = torch.empty_like(x)
        code = self._launch('instance_norm', lambda: self.lib.um_instance_norm_fwd(
            _ptr(x), _ptr(shortcut) if shortcut is not None else None, _ptr(y), n * c, h * w, float(eps),
            int(bool(relu)), _stream()))
        _abi.check(code, 'um_instance_norm_fwd')
        return y

    # ------------------------------------------------------------------ NHWC convolutions on the matrix cores
    # (also what the encoder uses).  An "NHWC activation" here is a small record:
    #   planes: operand planes [NS][rows + 1][C] (uint8 tensor; last row zero) or None
    #   f32   : fp32 [rows, C] or None;   b, h, w, c: geometry, rows = b * h * w
    def conv_weight_planes(self, weight):
        """Planes of an ``nn.Conv2d`` weight ``[cout, cin, kh, kw]`` permuted to ``[cout, kh*kw*cin]``; cached."""
        key, hit = self._cache_get('conv', (weight,))
        if hit is not None:
            return hit
        cout, cin, kh, kw = weight.shape
        w2 = weight.detach().float().permute(0, 2, 3, 1).reshape(cout, kh * kw * cin).contiguous()
        planes = torch.empty(self.lib.um_planes_bytes(cout, kh * kw * cin, self.CONV_MODE), dtype=torch.uint8, device=w2.device)
        self._check_weight_range(w2, self.WSHIFT, 'convolution weight')
        _abi.check(self.lib.um_weight_planes(_ptr(w2), _ptr(planes), cout, kh * kw * cin, self.WSHIFT, self.CONV_MODE, _stream()),
                   'um_weight_planes')
        return self._cache_put(key, (weight,), (planes, cout, cin, kh, kw))

    def conv2d_nhwc(self, act, weight, bias=None, stride=1, padding=(1, 1), relu=False, stats=False, image_addend=None):
        """``act``: ``(planes, b, h, w, cin)``; returns fp32 ``[b*ho*wo, cout]`` and ``(ho, wo)``.  With ``stats`` the epilogue also emits the per-tile InstanceNorm statistics: ``self.last_conv_stats``.
        ``image_addend``: fp32 ``[ho*wo, cout]``, one table added to every image's output in the epilogue (``um_conv2d_addend_fwd``,
        periodic form): bit for bit the plain result ``+ image_addend.repeat(b, 1)``; excludes ``relu`` and ``stats``."""
        planes, b, h, w, cin = act
        wp, cout, wcin, kh, kw = self.conv_weight_planes(weight)
        if wcin != cin:
            raise ValueError(f'conv2d_nhwc: weight expects {wcin} input channels, activation has {cin}')
        ph, pw = (padding, padding) if isinstance(padding, int) else padding
        ho, wo = (h + 2 * ph - kh) // stride + 1, (w + 2 * pw - kw) // stride + 1
        out = torch.empty((b * ho * wo, cout), dtype=torch.float32, device=planes.device)
        self.last_conv_stats = None
        if stats:                                    # (per-part statistics, parts per image): hand both to nhwc_norm(conv_stats=)
            parts = self.lib.um_conv_stats_parts(h, w, cout, kh, kw, stride, ph, pw)
            self.last_conv_stats = (torch.empty(self.lib.um_conv_stats_bytes(b, parts, cout) // 4, dtype=torch.float32,
                                                device=planes.device), parts)
        st = self.last_conv_stats[0] if self.last_conv_stats is not None else None
        meta = {'flops': 2.0 * b * ho * wo * cout * kh * kw * cin}
        if image_addend is not None:
            if relu or stats:
                raise ValueError('conv2d_nhwc: image_addend excludes relu and stats')
            if not (image_addend.is_cuda and image_addend.dtype == torch.float32 and image_addend.is_contiguous()
                    and tuple(image_addend.shape) == (ho * wo, cout)):
                raise ValueError(f'conv2d_nhwc: image_addend must be a contiguous CUDA float32 [{ho * wo}, {cout}] tensor, got '
                                 f'{tuple(image_addend.shape)} {image_addend.dtype}')
            code = self._launch('conv', lambda: self.lib.um_conv2d_addend_fwd(
                _ptr(planes), _ptr(wp), _ptr(bias) if bias is not None else None, _ptr(image_addend), cout, 1, _ptr(out),
                b, h, w, cin, cout, kh, kw, stride, ph, pw, self.WSHIFT, self.CONV_MODE, _stream()), meta)
            _abi.check(code, 'um_conv2d_addend_fwd')
            return out, ho, wo
        code = self._launch('conv', lambda: self.lib.um_conv2d_fwd(
            _ptr(planes), _ptr(wp), _ptr(bias) if bias is not None else None, _ptr(out), _ptr(st) if st is not None else None,
            b, h, w, cin, cout, kh, kw,
            stride, ph, pw, int(bool(relu)), self.WSHIFT, self.CONV_MODE, _stream()), meta)
        _abi.check(code, 'um_conv2d_fwd')
        return out, ho, wo

    def conv2d_norm_supported(self, h, w, cin, weight, stride=1, padding=(1, 1)):
        """True when ``conv2d_nhwc_normed`` serves this convolution (``um_conv2d_norm_supported``: a pure function of the geometry)."""
        cout, wcin, kh, kw = weight.shape
        ph, pw = (padding, padding) if isinstance(padding, int) else padding
        return wcin == cin and bool(self.lib.um_conv2d_norm_supported(h, w, cin, cout, kh, kw, stride, ph, pw, self.CONV_MODE))

    def conv2d_nhwc_normed(self, x, conv_stats, geom, weight, bias=None, norm_relu=True, relu=False, stats=False, eps=1e-5):
        """``conv2d_nhwc`` (3x3, stride 1, pad 1) of ``relu(instance_norm(x))`` where ``x`` is the fp32 NHWC output ``[b*h*w, cin]`` of
        the producing convolution and ``conv_stats`` the ``last_conv_stats`` it left: the statistics are finalized
        (``um_nhwc_stats_finalize``) and the convolution normalises while it stages its operand (``um_conv2d_norm_fwd``) -- the
        results of ``nhwc_norm`` + ``conv2d_nhwc`` bit for bit, without the normalisation's pass over memory."""
        b, h, w, cin = geom
        self._check_rows('x', x, cin)
        if x.shape[0] != b * h * w:
            raise ValueError('conv2d_nhwc_normed: x must have b * h * w rows')
        wp, cout, wcin, kh, kw = self.conv_weight_planes(weight)
        if wcin != cin:
            raise ValueError(f'conv2d_nhwc_normed: weight expects {wcin} input channels, activation has {cin}')
        nstats = torch.empty((b, 2, cin), dtype=torch.float32, device=x.device)          # per call: one buffer per stream lane
        _abi.check(self._launch('instance_norm', lambda: self.lib.um_nhwc_stats_finalize(
            _ptr(conv_stats[0]), conv_stats[1], _ptr(nstats), b, h * w, cin, float(eps), _stream())), 'um_nhwc_stats_finalize')
        out = torch.empty((b * h * w, cout), dtype=torch.float32, device=x.device)
        self.last_conv_stats = None
        if stats:
            parts = self.lib.um_conv_stats_parts(h, w, cout, kh, kw, 1, 1, 1)
            self.last_conv_stats = (torch.empty(self.lib.um_conv_stats_bytes(b, parts, cout) // 4, dtype=torch.float32,
                                                device=x.device), parts)
        st = self.last_conv_stats[0] if self.last_conv_stats is not None else None
        meta = {'flops': 2.0 * b * h * w * cout * kh * kw * cin}
        code = self._launch('conv', lambda: self.lib.um_conv2d_norm_fwd(
            _ptr(x), _ptr(nstats), int(bool(norm_relu)), _ptr(wp), _ptr(bias) if bias is not None else None, _ptr(out),
            _ptr(st) if st is not None else None, b, h, w, cin, cout, kh, kw, 1, 1, 1, int(bool(relu)), self.WSHIFT, self.CONV_MODE,
            _stream()), meta)
        _abi.check(code, 'um_conv2d_norm_fwd')
        return out, h, w

    def conv2d_entry_supported(self, h, w, cin, weight, proj_weight, stride=2, padding=(1, 1)):
        """True when ``conv2d_entry`` serves this transition block (``um_conv2d_entry_supported``: a pure function of the geometry)."""
        cout, wcin, kh, kw = weight.shape
        ph, pw = (padding, padding) if isinstance(padding, int) else padding
        return (wcin == cin and tuple(proj_weight.shape) == (cout, cin, 1, 1) and
                bool(self.lib.um_conv2d_entry_supported(h, w, cin, cout, kh, kw, stride, ph, pw, self.CONV_MODE)))

    def conv2d_entry(self, u, conv_stats, shortcut_planes, geom, weight, proj_weight, proj_bias, eps=1e-5):
        """A stride-2 residual block's entry in one launch (``um_conv2d_entry_fwd``): with ``X = relu(instance_norm(u) + shortcut)`` --
        the block input, which is never written -- returns ``(t, d, ho, wo, t_stats, d_stats)``: ``t = conv3x3/2(X)`` with ``weight``,
        ``d = conv1x1/2(X) + proj_bias`` and the ``last_conv_stats`` pair of each.  ``u`` is the fp32 NHWC output ``[b*h*w, cin]`` of the
        previous block's second convolution, ``conv_stats`` the pair it left, ``shortcut_planes`` that block's shortcut as operand
        planes.  Bit for bit ``nhwc_norm(u, shortcut_planes=)`` -> ``conv2d_nhwc`` twice."""
        b, h, w, cin = geom
        self._check_rows('u', u, cin)
        if u.shape[0] != b * h * w:
            raise ValueError('conv2d_entry: u must have b * h * w rows')
        if shortcut_planes.numel() != self.lib.um_planes_bytes(b * h * w + 1, cin, self.CONV_MODE):
            raise ValueError('conv2d_entry: shortcut_planes must be operand planes of [b * h * w + 1, cin]')
        wp, cout, wcin, kh, kw = self.conv_weight_planes(weight)
        wp2, cout2, wcin2, kh2, kw2 = self.conv_weight_planes(proj_weight)
        if wcin != cin or (cout2, wcin2, kh2, kw2) != (cout, cin, 1, 1):
            raise ValueError('conv2d_entry: the weights do not fit the activation / each other')
        nstats = torch.empty((b, 2, cin), dtype=torch.float32, device=u.device)          # per call: one buffer per stream lane
        _abi.check(self._launch('instance_norm', lambda: self.lib.um_nhwc_stats_finalize(
            _ptr(conv_stats[0]), conv_stats[1], _ptr(nstats), b, h * w, cin, float(eps), _stream())), 'um_nhwc_stats_finalize')
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        t = torch.empty((b * ho * wo, cout), dtype=torch.float32, device=u.device)
        d = torch.empty_like(t)
        parts = self.lib.um_conv_stats_parts(h, w, cout, 3, 3, 2, 1, 1)
        nst = self.lib.um_conv_stats_bytes(b, parts, cout) // 4
        st_t = torch.empty(nst, dtype=torch.float32, device=u.device)
        st_d = torch.empty(nst, dtype=torch.float32, device=u.device)
        meta = {'flops': 2.0 * b * ho * wo * cout * 10 * cin}
        code = self._launch('conv', lambda: self.lib.um_conv2d_entry_fwd(
            _ptr(u), _ptr(nstats), _ptr(shortcut_planes), _ptr(wp), _ptr(wp2), _ptr(proj_bias) if proj_bias is not None else None, _ptr(t), _ptr(d), _ptr(st_t), _ptr(st_d),
            b, h, w, cin, cout, 3, 3, 2, 1, 1, self.WSHIFT, self.CONV_MODE, _stream()), meta)
        _abi.check(code, 'um_conv2d_entry_fwd')
        self.last_conv_stats = (st_t, parts)
        return t, d, ho, wo, (st_t, parts), (st_d, parts)

    def nhwc_planes_from(self, pieces, pad_to=32):
        """Operand planes of the channel concatenation of fp32 NHWC pieces ``[rows, c_i]`` (zero-padded to a multiple of
        ``pad_to`` channels): returns ``(planes, channels)``."""
        rows = pieces[0].shape[0]
        c = sum(p.shape[1] for p in pieces)
        cp = (c + pad_to - 1) // pad_to * pad_to
        if cp != c:
            pieces = list(pieces) + [torch.zeros((rows, cp - c), dtype=torch.float32, device=pieces[0].device)]
        x = pieces[0].contiguous() if len(pieces) == 1 else torch.cat(list(pieces), 1)
        planes, _ = self.nhwc_norm(x, 1, rows, normalize=False, relu=False, want_planes=True)
        return planes, cp

    def nhwc_concat_planes(self, flow, tokens, pad_to=32):
        """``nhwc_planes_from([flow.permute(0, 2, 3, 1).reshape(rows, V), tokens])`` in one launch (``um_nhwc_concat_planes``): ``flow``
        fp32 ``[b, V, h, w]`` (V <= 4), ``tokens`` fp32 ``[b*h*w, C]`` -> ``(planes, channels)``, the same bytes."""
        if pad_to != 32:
            raise ValueError('nhwc_concat_planes: the kernel pads to 32 channels')
        b, v, h, w = flow.shape
        rows = b * h * w
        self._check_rows('tokens', tokens, tokens.shape[1])
        if not (flow.is_cuda and flow.dtype == torch.float32 and flow.is_contiguous() and tokens.shape[0] == rows):
            raise ValueError(f'nhwc_concat_planes: expected a contiguous CUDA float32 flow [b, V, h, w] and tokens [b*h*w, C], got '
                             f'{tuple(flow.shape)} {flow.dtype} and {tuple(tokens.shape)}')
        c = tokens.shape[1]
        cp = (v + c + 31) // 32 * 32
        planes = torch.empty(self.lib.um_planes_bytes(rows + 1, cp, self.CONV_MODE), dtype=torch.uint8, device=flow.device)
        code = self._launch('instance_norm', lambda: self.lib.um_nhwc_concat_planes(
            _ptr(flow), _ptr(tokens), _ptr(planes), b, h * w, v, c, self.CONV_MODE, _stream()))
        _abi.check(code, 'um_nhwc_concat_planes')
        return planes, cp

    def conv_weight_padded(self, weight, cin_to):
        """``weight [cout, cin, kh, kw]`` with zero input channels appended up to ``cin_to`` (cached by the caller's
        parameter identity through conv_weight_planes)."""
        key, hit = self._cache_get(('padw', cin_to), (weight,))
        if hit is None:
            cout, cin, kh, kw = weight.shape
            wpad = torch.zeros((cout, cin_to, kh, kw), dtype=torch.float32, device=weight.device)
            wpad[:, :cin] = weight.detach().float()
            hit = self._cache_put(key, (weight,), wpad)
        return hit

    # ---- building blocks of the channels-last refinement block (unimatch_amd/refine_nhwc.py) ---------------------------------
    def planes_buffer(self, rows, ld):
        """Zeroed operand-plane buffer ``[2][rows + 1][ld]`` (fp16 hi | lo); row ``rows`` is the zero padding row."""
        return torch.zeros(2 * (rows + 1) * ld * 2, dtype=torch.uint8, device='cuda')

    def cached_planes_buffer(self, tag, rows, ld, device):
        """A ``planes_buffer(rows, ld)`` allocated and zeroed once per (tag, geometry, device, owner) and handed out again (590 MB of
        zero-fill per forward at config 4 otherwise): only the padding row has to be zero and no kernel writes it.  One geometry per
        (tag, device, owner) stays resident."""
        return self._workspace(('planes', tag), (rows, ld), 2 * (rows + 1) * ld * 2, torch.device(device), 1)

    def conv_weight_planes_from(self, weight):
        """Uncached: planes of ``weight [cout, cin, kh, kw]`` permuted to ``[cout, kh*kw*cin]`` -> ``(planes, cout, cin, kh, kw)``."""
        cout, cin, kh, kw = weight.shape
        w2 = weight.detach().float().permute(0, 2, 3, 1).reshape(cout, kh * kw * cin).contiguous()
        planes = torch.empty(self.lib.um_planes_bytes(cout, kh * kw * cin, 0), dtype=torch.uint8, device=w2.device)
        self._check_weight_range(w2, self.WSHIFT, 'convolution weight')
        _abi.check(self.lib.um_weight_planes(_ptr(w2), _ptr(planes), cout, kh * kw * cin, self.WSHIFT, 0, _stream()),
                   'um_weight_planes')
        return planes, cout, cin, kh, kw

    def conv_ex(self, src, geom, wb, ksize, stride, pad, act, out=None, outp=None):
        """``um_conv2d_ex``.  ``src = (planes_buffer, ld, coff, cin)``, ``geom = (b, h, w)``, ``wb = ((w_planes, cout, cin, kh,
        kw), bias)``, ``out = (fp32 tensor, ld, coff)``, ``outp = (planes_buffer, ld, coff)``; act 0/1/2/3 = none/ReLU/sigmoid/tanh."""
        buf, a_ld, a_coff, cin = src
        b, h, w = geom
        (wp, cout, wcin, kh, kw), bias = wb
        if wcin != cin or (kh, kw) != tuple(ksize):
            raise ValueError(f'conv_ex: weight is {cout}x{wcin}x{kh}x{kw}, call wants cin={cin} k={ksize}')
        a_rows = buf.numel() // (4 * a_ld)
        ho, wo = (h + 2 * pad[0] - kh) // stride + 1, (w + 2 * pad[1] - kw) // stride + 1
        o_t, o_ld, o_coff = out if out is not None else (None, 0, 0)
        p_t, p_ld, p_coff = outp if outp is not None else (None, 0, 0)
        p_rows = p_t.numel() // (4 * p_ld) if p_t is not None else 0
        code = self._launch('conv', lambda: self.lib.um_conv2d_ex(
            _ptr(buf), a_ld, a_coff, a_rows, _ptr(wp), _ptr(bias) if bias is not None else None,
            _ptr(o_t) if o_t is not None else None, o_ld, o_coff, _ptr(p_t) if p_t is not None else None, p_ld, p_coff, p_rows,
            None, b, h, w, cin, cout, kh, kw, stride, pad[0], pad[1], act, self.WSHIFT, 0, _stream()),
            {'flops': 2.0 * b * ho * wo * cout * kh * kw * cin})
        _abi.check(code, 'um_conv2d_ex')

    def conv_gru(self, gate, src, geom, wb, ksize, pad, hidden, outp, z=None, z_out=None, addend=None, hidden_out=None):
        """``um_conv2d_gru_fwd``: gate 1 = (z | r) convolution -> ``z_out`` fp32 and ``r * hidden`` planes; gate 2 = q
        convolution -> ``hidden`` updated in place and written as planes.  ``src`` / ``wb`` / ``outp`` as :meth:`conv_ex`.
        ``addend``: fp32 ``[rows, cout]`` added before the gate's activation (``um_conv2d_gru_add_fwd``: the iteration-invariant
        input channels' share of the convolution, computed once per scale).  ``hidden_out`` (gate 2 with an addend): the new state goes
        there and ``hidden`` is only read."""
        buf, a_ld, a_coff, cin = src
        b, h, w = geom
        (wp, cout, wcin, kh, kw), bias = wb
        c = hidden.shape[1]
        if wcin != cin or (kh, kw) != tuple(ksize) or cout != (2 * c if gate == 1 else c):
            raise ValueError('conv_gru: weight / hidden shapes do not match')
        p_t, p_ld, p_coff = outp
        zt = z if gate == 2 else None
        if hidden_out is not None:
            if gate != 2 or addend is None or hidden_out.shape != hidden.shape or hidden_out.dtype != torch.float32 or not hidden_out.is_contiguous():
                raise ValueError('conv_gru: hidden_out goes with gate 2 and an addend, contiguous fp32 of the hidden state\'s shape')
            z_out = hidden_out
        if addend is not None:
            if not (addend.dtype == torch.float32 and addend.is_contiguous() and addend.dim() == 2 and addend.shape[1] == cout
                    and addend.shape[0] == geom[0] * geom[1] * geom[2]):
                raise ValueError(f'conv_gru: addend must be contiguous fp32 [b * h * w = {geom[0] * geom[1] * geom[2]}, cout = {cout}], '
                                 f'got {tuple(addend.shape)}')
            code = self._launch('conv', lambda: self.lib.um_conv2d_gru_add_fwd(
                gate, _ptr(buf), a_ld, a_coff, buf.numel() // (4 * a_ld), _ptr(wp), _ptr(bias) if bias is not None else None,
                _ptr(addend), addend.shape[1], _ptr(hidden), _ptr(zt) if zt is not None else None,
                zt.shape[1] if zt is not None else 0, _ptr(z_out) if z_out is not None else None,
                z_out.shape[1] if z_out is not None else 0, _ptr(p_t), p_ld, p_coff, p_t.numel() // (4 * p_ld), b, h, w, cin, c,
                kh, kw, pad[0], pad[1], self.WSHIFT, 0, _stream()), {'flops': 2.0 * b * h * w * cout * kh * kw * cin})
            _abi.check(code, 'um_conv2d_gru_add_fwd')
            return
        code = self._launch('conv', lambda: self.lib.um_conv2d_gru_fwd(
            gate, _ptr(buf), a_ld, a_coff, buf.numel() // (4 * a_ld), _ptr(wp), _ptr(bias) if bias is not None else None,
            _ptr(hidden), _ptr(zt) if zt is not None else None, zt.shape[1] if zt is not None else 0,
            _ptr(z_out) if z_out is not None else None, z_out.shape[1] if z_out is not None else 0, _ptr(p_t), p_ld, p_coff,
            p_t.numel() // (4 * p_ld), b, h, w, cin, c, kh, kw, pad[0], pad[1], self.WSHIFT, 0, _stream()),
            {'flops': 2.0 * b * h * w * cout * kh * kw * cin})
        _abi.check(code, 'um_conv2d_gru_fwd')

    def conv7(self, image, weight, bias, stride, act, out=None, outp=None):
        """7x7 / pad 3 convolution of an fp32 NCHW image with few channels (``um_conv7_fwd``), outputs as :meth:`conv_ex`."""
        b, c, h, w = image.shape
        cout = weight.shape[0]
        cpp = 4 if stride == 2 else 8
        key, hit = self._cache_get(('conv7', stride), (weight,))
        if hit is None:
            wr = torch.zeros((cout, 7, 8, cpp), dtype=torch.float32, device=weight.device)
            wr[:, :, :7, :c] = weight.detach().float().permute(0, 2, 3, 1)
            wr = wr.reshape(cout, 56 * cpp).contiguous()
            wp = torch.empty(self.lib.um_planes_bytes(cout, 56 * cpp, 0), dtype=torch.uint8, device=weight.device)
            self._check_weight_range(wr, self.WSHIFT, 'convolution weight')
            _abi.check(self.lib.um_weight_planes(_ptr(wr), _ptr(wp), cout, 56 * cpp, self.WSHIFT, 0, _stream()), 'um_weight_planes')
            hit = self._cache_put(key, (weight,), wp)
        scratch = torch.empty(self.lib.um_conv7_planes_bytes(b, h, w, stride), dtype=torch.uint8, device=image.device)
        o_t, o_ld, o_coff = out if out is not None else (None, 0, 0)
        p_t, p_ld, p_coff = outp if outp is not None else (None, 0, 0)
        p_rows = p_t.numel() // (4 * p_ld) if p_t is not None else 0
        image = image.contiguous()
        code = self._launch('conv', lambda: self.lib.um_conv7_fwd(
            _ptr(image), c, 0, None, None, _ptr(scratch), _ptr(hit), _ptr(bias) if bias is not None else None,
            _ptr(o_t) if o_t is not None else None, o_ld, o_coff, _ptr(p_t) if p_t is not None else None, p_ld, p_coff, p_rows,
            None, b, h, w, cout, stride, act, self.WSHIFT, _stream()))
        _abi.check(code, 'um_conv7_fwd')

    def nhwc_gate(self, mode, src, dest, ld, coff, rows, channels, zr=None, hbuf=None):
        """``um_nhwc_gate``: column scatter (0), ``r * h`` (1), GRU state update (2) into ``dest`` planes ``[2][.][ld]``."""
        p_rows = dest.numel() // (4 * ld) if dest is not None else 0
        src_ld = src.shape[1] if src is not None else 0
        code = self._launch('instance_norm', lambda: self.lib.um_nhwc_gate(
            mode, _ptr(src) if src is not None else None, src_ld, _ptr(zr) if zr is not None else None,
            _ptr(hbuf) if hbuf is not None else None, _ptr(dest) if dest is not None else None, ld, coff, p_rows, rows, channels,
            _stream()))
        _abi.check(code, 'um_nhwc_gate')

    def local_corr_with_flow_planes(self, f0, f1, flow, h, w, radius, dest, ld):
        """K4 written channels-last as operand planes (``um_local_corr_with_flow_planes``)."""
        b, l, c = f0.shape
        _check_tokens('f0', f0, tokens=h * w)
        _check_tokens('f1', f1, b, l)
        _check_map('flow', flow, b, h, w)
        if flow.shape[1] != 2:
            raise ValueError('flow must have 2 channels')
        # the kernel writes rows 0 .. b*h*w-1 of both planes and the convolutions read the zero padding row after them
        if not (torch.is_tensor(dest) and dest.is_cuda and dest.dtype == torch.uint8 and dest.is_contiguous() and ld > 0
                and dest.numel() // (4 * ld) >= b * l + 1):
            raise ValueError(f'dest: expected a contiguous CUDA uint8 planes buffer of at least ({b * l} + 1) x {ld} fp16 elements per '
                             f'plane (planes_buffer(rows, ld)), got {tuple(dest.shape) if torch.is_tensor(dest) else type(dest).__name__} '
                             f'{getattr(dest, "dtype", None)}')
        feat = self._k4_feat_planes(f0, f1, h, w, radius)
        if feat is not None:
            code = self._launch('local_corr_with_flow', lambda: self.lib.um_local_corr_with_flow_feat(
                _ptr(f0), _ptr(f1), _ptr(feat), _ptr(flow), None, _ptr(dest), ld, dest.numel() // (4 * ld), b, h, w, c, radius,
                self.k4_flags, None, _stream()))
            _abi.check(code, 'um_local_corr_with_flow_feat')
            return
        code = self._launch('local_corr_with_flow', lambda: self.lib.um_local_corr_with_flow_planes(
            _ptr(f0), _ptr(f1), _ptr(flow), _ptr(dest), ld, dest.numel() // (4 * ld), b, h, w, c, radius, _stream()))
        _abi.check(code, 'um_local_corr_with_flow_planes')

    # Cost-volume dispatch is a PURE FUNCTION of the call's arguments: radius 4 on a map of whole 8 x 4 pixel tiles goes to the
    # matrix-core kernel (k4m_kernel), whose own per-tile test -- does the tile's flow fit one 32 x 24 window? -- picks the
    # product path or the gather path from the flow values alone; every other geometry goes to the VALU kernel.  Two forwards
    # on the same inputs therefore run the same instructions (bitwise-equal outputs, HIP-graph capture freezes nothing).
    # Round 2 routed launches by a tile-coherence counter read back asynchronously; that made the choice timing dependent
    # for ~3 % on incoherent flow (k4m's gather path 0.661 ms against 0.643 ms at 4 x 128 x 192) and is gone.
    k4_mfma = True             # False: VALU kernels everywhere (tests compare the two; tools A/B them)
    k4_flags = 0               # bit 0: force k4m_kernel's per-pixel path for every tile (diagnostics)

    def _k4_feat_planes(self, f0, f1, h, w, radius):
        """fp16 hi | lo operand planes of (f0, f1) for um_local_corr_with_flow_feat, or None where that kernel does not apply.
        The refinement loop passes the same two tensors in every iteration: one entry, keyed by identity and version."""
        if not self.k4_mfma or not self.lib.um_local_corr_with_flow_feat_supported(h, w, f0.shape[2], radius):
            return None
        key = (id(f0), f0._version, f0.data_ptr(), id(f1), f1._version, f1.data_ptr(), tuple(f0.shape))
        hit = getattr(self, '_k4_feat', None)
        if hit is not None and hit[0] == key and hit[1]() is f0 and hit[2]() is f1:
            return hit[3]
        b, l, c = f0.shape
        feat = torch.empty(self.lib.um_local_corr_feat_planes_bytes(b, h, w, c), dtype=torch.uint8, device=f0.device)
        _abi.check(self.lib.um_local_corr_feat_planes(_ptr(f0), _ptr(f1), _ptr(feat), b, h, w, c, _stream()),
                   'um_local_corr_feat_planes')
        self._k4_feat = (key, weakref.ref(f0), weakref.ref(f1), feat)
        return feat

    def stem_conv(self, image, weight, norm_mean_std=None, stats=True):
        """The encoder's 7x7/2 stem on ``um_stem_conv_fwd``: fp32 NCHW image ``[b,3,h,w]`` -> fp32 NHWC ``[b*ho*wo, cout]``.
        ``norm_mean_std``: ``((m0,m1,m2), (s0,s1,s2))`` applies the reference's ``(x / 255 - mean) / std`` while packing.
        ``image`` may be a tuple of two such tensors of one size: the stem of their concatenation, which is never built
        (``um_stem_conv_pair_fwd``)."""
        pair = None
        if isinstance(image, (tuple, list)):
            pair = tuple(image)
            if len(pair) != 2 or pair[0].shape[1:] != pair[1].shape[1:] or pair[0].device != pair[1].device:
                raise ValueError('stem_conv: a tuple holds two image tensors of one size on one device')
            for im in pair[1:]:
                if not (im.is_cuda and im.dtype == torch.float32 and im.dim() == 4 and im.shape[1] == 3 and im.is_contiguous()):
                    raise ValueError('stem_conv: expected a contiguous CUDA float32 [b, 3, h, w] image')
            image = pair[0]
        if not (image.is_cuda and image.dtype == torch.float32 and image.dim() == 4 and image.shape[1] == 3
                and image.is_contiguous()):
            raise ValueError('stem_conv: expected a contiguous CUDA float32 [b, 3, h, w] image')
        if tuple(weight.shape[1:]) != (3, 7, 7):
            raise ValueError('stem_conv: expected a [cout, 3, 7, 7] weight')
        b, _, h, w = image.shape
        if pair is not None:
            b += pair[1].shape[0]
        cout = weight.shape[0]
        key, hit = self._cache_get('stem', (weight,))
        if hit is None:
            wr = torch.zeros((cout, 7, 8, 4), dtype=torch.float32, device=weight.device)
            wr[:, :, :7, :3] = weight.detach().float().permute(0, 2, 3, 1)
            wr = wr.reshape(cout, 224).contiguous()
            wp = torch.empty(self.lib.um_planes_bytes(cout, 224, 0), dtype=torch.uint8, device=weight.device)
            self._check_weight_range(wr, self.WSHIFT, 'convolution weight')
            _abi.check(self.lib.um_weight_planes(_ptr(wr), _ptr(wp), cout, 224, self.WSHIFT, 0, _stream()), 'um_weight_planes')
            hit = self._cache_put(key, (weight,), wp)
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        scratch = torch.empty(self.lib.um_stem_planes_bytes(b, h, w), dtype=torch.uint8, device=image.device)
        out = torch.empty((b * ho * wo, cout), dtype=torch.float32, device=image.device)
        self.last_conv_stats = None
        if stats:
            parts = self.lib.um_conv_stats_parts(h, w, cout, 7, 7, 2, 3, 3)
            self.last_conv_stats = (torch.empty(self.lib.um_conv_stats_bytes(b, parts, cout) // 4, dtype=torch.float32,
                                                device=image.device), parts)
        st = self.last_conv_stats[0] if self.last_conv_stats is not None else None
        if norm_mean_std is not None:
            mean = (ctypes.c_float * 3)(*[float(v) for v in norm_mean_std[0]])
            std = (ctypes.c_float * 3)(*[float(v) for v in norm_mean_std[1]])
        else:
            mean = std = None
        meta = {'flops': 2.0 * b * ho * wo * cout * 147}
        if pair is not None:
            code = self._launch('conv', lambda: self.lib.um_stem_conv_pair_fwd(
                _ptr(pair[0]), pair[0].shape[0], _ptr(pair[1]), pair[1].shape[0], int(norm_mean_std is not None), mean, std,
                _ptr(scratch), _ptr(hit), _ptr(out), _ptr(st) if st is not None else None, h, w, cout, self.WSHIFT, _stream()), meta)
            _abi.check(code, 'um_stem_conv_pair_fwd')
            return out, ho, wo
        code = self._launch('conv', lambda: self.lib.um_stem_conv_fwd(
            _ptr(image), int(norm_mean_std is not None), mean, std, _ptr(scratch), _ptr(hit), _ptr(out),
            _ptr(st) if st is not None else None, b, h, w, cout, self.WSHIFT, _stream()), meta)
        _abi.check(code, 'um_stem_conv_fwd')
        return out, ho, wo

    def nhwc_norm(self, x, b, pixels, normalize=True, relu=True, shortcut=None, want_planes=True, want_f32=False, eps=1e-5,
                  conv_stats=None, shortcut_planes=None, shortcut_stats=None):
        """InstanceNorm (+ ReLU, + shortcut + ReLU) of fp32 NHWC ``x [b*pixels, c]`` -> ``(planes | None, f32 | None)``.
        The shortcut is fp32 ``[b*pixels, c]`` or (``shortcut_planes``) operand planes of the same shape; ``conv_stats`` is the
        ``(statistics, parts per image)`` pair the producing convolution left in ``last_conv_stats``.  ``shortcut_stats``: such a
        pair for an fp32 ``shortcut`` that is a projection's raw output -- its own InstanceNorm is applied on load
        (``um_nhwc_instance_norm_sc``) instead of in a pass of its own."""
        self._check_rows('x', x, x.shape[1])
        c = x.shape[1]
        if x.shape[0] != b * pixels:
            raise ValueError('nhwc_norm: x must have b * pixels rows')
        if shortcut is not None:
            self._check_rows('shortcut', shortcut, c)
        rows = b * pixels
        if shortcut_planes is not None and (shortcut is not None or shortcut_planes.numel() != self.lib.um_planes_bytes(rows + 1, c, self.CONV_MODE)):
            raise ValueError('nhwc_norm: shortcut_planes must be operand planes of [b * pixels + 1, c] (and exclude shortcut)')
        planes = (torch.empty(self.lib.um_planes_bytes(rows + 1, c, self.CONV_MODE), dtype=torch.uint8, device=x.device)
                  if want_planes else None)
        f32 = torch.empty_like(x) if want_f32 else None
        if shortcut_stats is not None:
            if shortcut is None or not normalize:
                raise ValueError('nhwc_norm: shortcut_stats go with an fp32 shortcut and normalize=True')
            ws = self._ws(self.lib.um_nhwc_norm_sc_workspace_bytes(b, pixels, c), x.device)
            code = self._launch('instance_norm', lambda: self.lib.um_nhwc_instance_norm_sc(
                _ptr(x), _ptr(shortcut), None, _ptr(planes) if planes is not None else None,
                _ptr(f32) if f32 is not None else None, b, pixels, c, float(eps), 1, int(bool(relu)),
                _ptr(conv_stats[0]) if conv_stats is not None else None, conv_stats[1] if conv_stats is not None else 0,
                _ptr(ws), ws.numel(), self.CONV_MODE, _stream(), _ptr(shortcut_stats[0]), shortcut_stats[1]))
            _abi.check(code, 'um_nhwc_instance_norm_sc')
            return planes, f32
        ws = self._ws(self.lib.um_nhwc_norm_workspace_bytes(b, pixels, c), x.device) if normalize else None
        code = self._launch('instance_norm', lambda: self.lib.um_nhwc_instance_norm(
            _ptr(x), _ptr(shortcut) if shortcut is not None else None,
            _ptr(shortcut_planes) if shortcut_planes is not None else None, _ptr(planes) if planes is not None else None,
            _ptr(f32) if f32 is not None else None, b, pixels, c, float(eps), int(bool(normalize)), int(bool(relu)),
            _ptr(conv_stats[0]) if conv_stats is not None else None, conv_stats[1] if conv_stats is not None else 0,
            _ptr(ws) if ws is not None else None, ws.numel() if ws is not None else 0, self.CONV_MODE, _stream()))
        _abi.check(code, 'um_nhwc_instance_norm')
        return planes, f32

    def nchw_to_nhwc(self, x, want_planes=True, want_f32=False):
        """fp32 NCHW map -> NHWC operand planes and / or fp32 ``[b*h*w, c]``."""
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
            raise ValueError('nchw_to_nhwc: expected a contiguous CUDA float32 NCHW tensor')
        b, c, h, w = x.shape
        rows = b * h * w
        planes = (torch.empty(self.lib.um_planes_bytes(rows + 1, c, self.CONV_MODE), dtype=torch.uint8, device=x.device)
                  if want_planes else None)
        f32 = torch.empty((rows, c), dtype=torch.float32, device=x.device) if want_f32 else None
        code = self._launch('instance_norm', lambda: self.lib.um_nchw_to_nhwc(
            _ptr(x), _ptr(planes) if planes is not None else None, _ptr(f32) if f32 is not None else None, b, c, h * w,
            self.CONV_MODE, _stream()))
        _abi.check(code, 'um_nchw_to_nhwc')
        return planes, f32

    # ------------------------------------------------------------------ global matching
    def global_corr_softmax_flow(self, f0, f1, h, w, bidir=False):
        b, l, c = f0.shape
        _check_tokens('f0', f0, tokens=h * w)
        _check_tokens('f1', f1, b, l)
        out = torch.empty((2 * b if bidir else b, 2, h, w), dtype=torch.float32, device=f0.device)
        ws = self._ws(self.lib.um_global_corr_workspace_bytes(b, l, c, self.mode), f0.device)
        meta = {'flops': (2.0 if bidir else 1.0) * b * (2.0 * l * l * c + 4.0 * l * l),
                'bytes': 2.0 * 4 * b * l * c + 8.0 * b * l}
        code = self._launch('global_corr_flow', lambda: self.lib.um_global_corr_softmax_flow(
            _ptr(f0), _ptr(f1), _ptr(out), b, h, w, c, int(bool(bidir)), self.mode,
            _ptr(ws), ws.numel(), _stream()), meta)
        _abi.check(code, 'um_global_corr_softmax_flow')
        return out

    def global_corr_softmax_stereo(self, f0, f1, h, w):
        b, l, c = f0.shape
        _check_tokens('f0', f0, tokens=h * w)
        _check_tokens('f1', f1, b, l)
        out = torch.empty((b, 1, h, w), dtype=torch.float32, device=f0.device)
        ws = self._ws(self.lib.um_global_corr_workspace_bytes(b, l, c, self.mode), f0.device)
        code = self._launch('global_corr_stereo', lambda: self.lib.um_global_corr_softmax_stereo(
            _ptr(f0), _ptr(f1), _ptr(out), b, h, w, c, self.mode, _ptr(ws), ws.numel(), _stream()))
        _abi.check(code, 'um_global_corr_softmax_stereo')
        return out

    def prop_global(self, q, k, value, h, w):
        b, l, c = q.shape
        _check_tokens('q', q, tokens=h * w)
        _check_tokens('k', k, b, l)
        _check_map('value', value, b, h, w)
        out = torch.empty_like(value)
        ws = self._ws(self.lib.um_global_corr_workspace_bytes(b, l, c, self.mode), q.device)
        vch = value.shape[1]
        meta = {'flops': b * (2.0 * l * l * c + 2.0 * l * l * vch), 'bytes': 2.0 * 4 * b * l * c + 8.0 * b * l * vch}
        code = self._launch('prop_global', lambda: self.lib.um_prop_global_attn(
            _ptr(q), _ptr(k), _ptr(value), _ptr(out), b, h, w, c, vch, self.mode,
            _ptr(ws), ws.numel(), _stream()), meta)
        _abi.check(code, 'um_prop_global_attn')
        return out

    def linear_bias(self, a, weight, bias, out_mul=1.0, bias_mul=1.0, planes=False, a_planes_k=None):
        """``nn.Linear`` with bias on ``um_linear_bias_fwd``: ``(A . W^T) * out_mul + bias * bias_mul`` as fp32 ``[M, N]`` or
        (``planes``) as MFMA operand planes.  ``a``: fp32 ``[M, K]``, or planes with ``a_planes_k`` columns."""
        wp, n, k = self.weight_planes((weight,))
        if a_planes_k is not None:
            m = a.numel() // (2 * self.nplanes * a_planes_k)
            src = (None, _ptr(a))
        else:
            m = a.shape[0]
            self._check_rows('a', a, k)
            src = (_ptr(a), None)
        bias = bias.detach()
        if not (bias.is_cuda and bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == n):
            raise ValueError(f'linear_bias: expected a contiguous CUDA float32 bias of {n} elements')
        if planes:
            out = torch.empty(self.lib.um_planes_bytes(m, n, self.mode), dtype=torch.uint8, device=a.device)
            dst = (_ptr(out), None)
        else:
            out = torch.empty((m, n), dtype=torch.float32, device=a.device)
            dst = (None, _ptr(out))
        code = self._launch('linear', lambda: self.lib.um_linear_bias_fwd(
            src[0], src[1], _ptr(wp), _ptr(bias), m, n, k, self.WSHIFT, float(out_mul), float(bias_mul), dst[0], dst[1],
            self.mode, _stream()), {'flops': 2.0 * m * n * k})
        _abi.check(code, 'um_linear_bias_fwd')
        return out

    def prop_global_projected(self, tokens, q_proj, k_proj, value, h, w):
        """The whole global propagation layer (attention.py:196-213): ``q = Wq x + bq``, ``k = Wk q + bk`` (of q -- the
        reference's quirk), ``softmax(q k^T / sqrt(C)) value``.  q and k go from the projection kernels to the attention
        kernel as operand planes; no library GEMM, no fp32 q / k."""
        b, l, c = tokens.shape
        _check_tokens('tokens', tokens, tokens=h * w)
        _check_map('value', value, b, h, w)
        ps = self.lib.um_global_corr_plane_scale(c)
        x = tokens.reshape(b * l, c)
        qp = self.linear_bias(x, q_proj.weight, q_proj.bias, out_mul=ps, bias_mul=ps, planes=True)
        kp = self.linear_bias(qp, k_proj.weight, k_proj.bias, out_mul=1.0, bias_mul=ps, planes=True, a_planes_k=c)
        out = torch.empty_like(value)
        ws = self._ws(self.lib.um_global_corr_workspace_bytes(b, l, c, self.mode), tokens.device)
        vch = value.shape[1]
        meta = {'flops': b * (2.0 * l * l * c + 2.0 * l * l * vch), 'bytes': 2.0 * 4 * b * l * c + 8.0 * b * l * vch}
        code = self._launch('prop_global', lambda: self.lib.um_prop_global_attn_planes(
            _ptr(qp), _ptr(kp), _ptr(value), _ptr(out), b, h, w, c, vch, self.mode, _ptr(ws), ws.numel(), _stream()), meta)
        _abi.check(code, 'um_prop_global_attn_planes')
        return out

    # ------------------------------------------------------------------ local kernels (fp32)
    def local_corr_softmax(self, f0, f1, h, w, radius, one_d=False):
        b, l, c = f0.shape
        _check_tokens('f0', f0, tokens=h * w)
        _check_tokens('f1', f1, b, l)
        out = torch.empty((b, 1 if one_d else 2, h, w), dtype=torch.float32, device=f0.device)
        if not one_d and self.k4_mfma and self.lib.um_local_corr_with_flow_feat_supported(h, w, c, radius):
            ws = self._ws(self.lib.um_local_corr_feat_planes_bytes(b, h, w, c), f0.device)
            code = self._launch('local_corr_softmax', lambda: self.lib.um_local_corr_softmax_mfma(
                _ptr(f0), _ptr(f1), _ptr(out), b, h, w, c, radius, _ptr(ws), ws.numel(), _stream()))
            _abi.check(code, 'um_local_corr_softmax_mfma')
            return out
        code = self._launch('local_corr_softmax', lambda: self.lib.um_local_corr_softmax(
            _ptr(f0), _ptr(f1), _ptr(out), b, h, w, c, radius, int(bool(one_d)), _stream()))
        _abi.check(code, 'um_local_corr_softmax')
        return out

    def local_corr_with_flow(self, f0, f1, flow, h, w, radius, dilation=1):
        """``local_correlation_with_flow`` (matching.py:86-123) -> ``[B, (2r+1)^2, h, w]``; ``dilation`` as in the reference
        (1 everywhere in its callers; other values take ``um_local_corr_with_flow_dilated``'s plain gather)."""
        b, l, c = f0.shape
        _check_tokens('f0', f0, tokens=h * w)
        _check_tokens('f1', f1, b, l)
        _check_map('flow', flow, b, h, w)
        if flow.shape[1] != 2:
            raise ValueError('flow must have 2 channels')
        k = 2 * radius + 1
        out = torch.empty((b, k * k, h, w), dtype=torch.float32, device=f0.device)
        meta = {'flops': 2.0 * b * l * (k + 1) ** 2 * c, 'bytes': 2.0 * 4 * b * l * c + 8.0 * b * l + 4.0 * k * k * b * l}
        if dilation != 1:
            code = self._launch('local_corr_with_flow', lambda: self.lib.um_local_corr_with_flow_dilated(
                _ptr(f0), _ptr(f1), _ptr(flow.contiguous()), _ptr(out), b, h, w, c, radius, int(dilation), _stream()), meta)
            _abi.check(code, 'um_local_corr_with_flow_dilated')
            return out
        feat = self._k4_feat_planes(f0, f1, h, w, radius)
        if feat is not None:
            code = self._launch('local_corr_with_flow', lambda: self.lib.um_local_corr_with_flow_feat(
                _ptr(f0), _ptr(f1), _ptr(feat), _ptr(flow), _ptr(out), None, 0, 0, b, h, w, c, radius, self.k4_flags,
                None, _stream()), meta)
            _abi.check(code, 'um_local_corr_with_flow_feat')
            return out
        code = self._launch('local_corr_with_flow', lambda: self.lib.um_local_corr_with_flow(
            _ptr(f0), _ptr(f1), _ptr(flow), _ptr(out), b, h, w, c, radius, _stream()), meta)
        _abi.check(code, 'um_local_corr_with_flow')
        return out

    def prop_local(self, q, k, value, h, w, radius):
        b, l, c = q.shape
        _check_tokens('q', q, tokens=h * w)
        _check_tokens('k', k, b, l)
        _check_map('value', value, b, h, w)
        out = torch.empty_like(value)
        code = self._launch('prop_local', lambda: self.lib.um_prop_local_attn(
            _ptr(q), _ptr(k), _ptr(value), _ptr(out), b, h, w, c, value.shape[1], radius, _stream()))
        _abi.check(code, 'um_prop_local_attn')
        return out

    def depth_corr_softmax(self, f0, f1, h, w, cam, candidates, from_argmax=False, stats=False, peak_radius=1, use=None, rows=None):
        """cam ``[B, 30]`` = K^-1 | R | t | K (row major), candidates ``[D]`` inverse depths -> ``out [B, 1, h, w]``.

        ``stats=True``: the same sweep as ONE ``um_depth_corr_softmax_stats`` launch (recorded as ``'depth_corr_softmax_stats'``) that
        also writes the statistics of the distribution it reduces -> ``(out, stats [B, 4, h, w] = max_prob | entropy | variance |
        peak_mass, index [B, 2, h, w] int32 = best | in_view)``; ``peak_radius``: candidates each side of the best one that count
        towards ``peak_mass``.  Its memory-contract cases are in tests/test_depth_stats_gpu.py.

        Source-major ``f0``, ``f1`` ``[S, B, h*w, 128]`` with ``cam [S, B, 30]``: the S views vote in ONE plane sweep
        (``um_depth_corr_softmax_multi``, recorded as ``'depth_corr_softmax_multi'``; ``use [S, B]`` switches views off per sample): see
        :meth:`_depth_corr_softmax_multi`; its memory-contract cases are in tests/test_depth_multiview_gpu.py.  Why one method has two
        layouts chosen by the rank of ``f0`` instead of a public ``depth_corr_softmax_multi``: the public method list of this class is
        pinned by tests/test_memory_contract_gpu.py (every public method needs a case or a reason in that file's tables), so a new
        launch of an existing operation comes in through the existing method, as ``stats=True`` did.

        ``rows [S, B, 3]`` int32 on the device: the same fused sweep on operands that are ROWS of other tensors
        (``um_depth_corr_softmax_multi_rows``, recorded as ``'depth_corr_softmax_multi_rows'``).  ``f0`` is then a tuple or list of 1 .. 4
        token tensors ``[n_i, h*w, 128]`` (the segments a token row indexes, concatenated in order), ``f1`` is None and ``cam`` is
        ``[Rc, 30]``: see :meth:`_depth_corr_softmax_multi_rows`; its memory-contract cases are in
        tests/test_depth_fuse_neighbours_gpu.py."""
        if rows is not None:
            if f1 is not None or use is not None:
                raise ValueError('rows names every operand: f1 must be None (f0 holds the segments) and use must be None (an off source has a negative row)')
            return self._depth_corr_softmax_multi_rows(f0, h, w, cam, rows, candidates, from_argmax, stats, peak_radius)
        if f0.dim() == 4:
            return self._depth_corr_softmax_multi(f0, f1, h, w, cam, candidates, use, from_argmax, stats, peak_radius)
        if use is not None:
            raise ValueError('use switches source views off: it needs source-major features [S, B, h*w, C]')
        b, l, c = f0.shape
        _check_tokens('f0', f0, tokens=h * w)
        _check_tokens('f1', f1, b, l)
        if not (cam.is_cuda and cam.dtype == torch.float32 and cam.is_contiguous() and tuple(cam.shape) == (b, 30)):
            raise ValueError(f'cam: expected contiguous CUDA float32 [{b}, 30]')
        if not (candidates.is_cuda and candidates.dtype == torch.float32 and candidates.is_contiguous()
                and candidates.dim() == 1):
            raise ValueError('candidates: expected contiguous CUDA float32 [D]')
        out = torch.empty((b, 1, h, w), dtype=torch.float32, device=f0.device)
        if stats:
            planes = torch.empty((b, 4, h, w), dtype=torch.float32, device=f0.device)
            index = torch.empty((b, 2, h, w), dtype=torch.int32, device=f0.device)
            code = self._launch('depth_corr_softmax_stats', lambda: self.lib.um_depth_corr_softmax_stats(
                _ptr(f0), _ptr(f1), _ptr(cam), _ptr(candidates), _ptr(out), _ptr(planes), _ptr(index), b, h, w, c,
                candidates.numel(), int(bool(from_argmax)), int(peak_radius), _stream()))
            _abi.check(code, 'um_depth_corr_softmax_stats')
            return out, planes, index
        code = self._launch('depth_corr_softmax', lambda: self.lib.um_depth_corr_softmax(
            _ptr(f0), _ptr(f1), _ptr(cam), _ptr(candidates), _ptr(out), b, h, w, c,
            candidates.numel(), int(bool(from_argmax)), _stream()))
        _abi.check(code, 'um_depth_corr_softmax')
        return out

    def _depth_corr_softmax_multi(self, f0, f1, h, w, cam, candidates, use=None, from_argmax=False, stats=False, peak_radius=1):
        """:meth:`depth_corr_softmax` for source-major inputs (a private name: the public method is the one entry of the plane sweep).
        The plane sweep with ``S`` source views voting in one cost volume (``um_depth_corr_softmax_multi``, csrc/depth_multi.hip):
        source-major ``f0``, ``f1`` ``[S, B, h*w, 128]``, ``cam [S, B, 30]``, ``use [S, B]`` uint8 / bool on the device (0: the source is
        off for that sample and is never read) or None -> ``out [B, 1, h, w]``; ``stats=True`` -> ``(out, stats [B, 4, h, w], index
        [B, 2, h, w] int32)`` as :meth:`depth_corr_softmax`.  The logits are averaged over the sources that see a candidate, then one
        softmax: an unlearned extension.  ONE launch, recorded as ``'depth_corr_softmax_multi'``; no host synchronisation."""
        if f0.dim() != 4 or not 1 <= f0.shape[0] <= 8:
            raise ValueError(f'f0: expected source-major [S = 1 .. 8, B, h*w, C], got {tuple(f0.shape)}')
        s, b, l, c = f0.shape
        for name, t in (('f0', f0), ('f1', f1)):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (s, b, h * w, c)):
                raise ValueError(f'{name}: expected a contiguous CUDA float32 [{s}, {b}, {h * w}, {c}] tensor, got '
                                 f'{tuple(t.shape)} {t.dtype} {t.device} contiguous={t.is_contiguous()}')
        if not (cam.is_cuda and cam.dtype == torch.float32 and cam.is_contiguous() and tuple(cam.shape) == (s, b, 30)):
            raise ValueError(f'cam: expected contiguous CUDA float32 [{s}, {b}, 30]')
        if not (candidates.is_cuda and candidates.dtype == torch.float32 and candidates.is_contiguous()
                and candidates.dim() == 1):
            raise ValueError('candidates: expected contiguous CUDA float32 [D]')
        if use is not None:
            if not (use.is_cuda and use.dtype in (torch.uint8, torch.bool) and use.is_contiguous() and tuple(use.shape) == (s, b)):
                raise ValueError(f'use: expected contiguous CUDA uint8 or bool [{s}, {b}]')
        out = torch.empty((b, 1, h, w), dtype=torch.float32, device=f0.device)
        planes = torch.empty((b, 4, h, w), dtype=torch.float32, device=f0.device) if stats else None
        index = torch.empty((b, 2, h, w), dtype=torch.int32, device=f0.device) if stats else None
        code = self._launch('depth_corr_softmax_multi', lambda: self.lib.um_depth_corr_softmax_multi(
            _ptr(f0), _ptr(f1), _ptr(cam), _ptr(use) if use is not None else None, _ptr(candidates), _ptr(out),
            _ptr(planes) if stats else None, _ptr(index) if stats else None, s, b, h, w, c,
            candidates.numel(), int(bool(from_argmax)), int(peak_radius), _stream()))
        _abi.check(code, 'um_depth_corr_softmax_multi')
        return (out, planes, index) if stats else out

    def _depth_corr_softmax_multi_rows(self, segments, h, w, cam, rows, candidates, from_argmax=False, stats=False, peak_radius=1):
        """:meth:`depth_corr_softmax` with a row table (a private name, as :meth:`_depth_corr_softmax_multi`): the fused plane sweep of
        ``S`` source views per sample whose operands are rows of the ``segments`` (1 .. 4 contiguous CUDA float32 tensors ``[n_i, h*w,
        128]``; a token row indexes their concatenation in order) and of ``cam [Rc, 30]``.  ``rows [S, B, 3]`` int32 on the device =
        f0 row | f1 row | cam row; a source with a negative or too-large index is off for that sample and is never read, so no table
        can make the kernel read out of bounds.  Returns what :meth:`_depth_corr_softmax_multi` returns, bit for bit its result on the
        same operands copied into the source-major layout.  ONE launch, recorded as ``'depth_corr_softmax_multi_rows'``; the host does
        not look at ``rows``: no synchronisation."""
        if torch.is_tensor(segments) or not 1 <= len(segments) <= 4:
            raise ValueError('rows: f0 must be a tuple or list of 1 .. 4 token tensors (the segments)')
        l = h * w
        for i, t in enumerate(segments):
            if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous() and t.shape[0] >= 1
                    and tuple(t.shape[1:]) == (l, 128) and t.device == segments[0].device):
                raise ValueError(f'segment {i}: expected a contiguous CUDA float32 [n >= 1, {l}, 128] tensor on {segments[0].device}, got '
                                 f'{tuple(t.shape)} {t.dtype} {t.device} contiguous={t.is_contiguous()}')
        dev = segments[0].device
        if not (cam.is_cuda and cam.dtype == torch.float32 and cam.is_contiguous() and cam.dim() == 2 and cam.shape[0] >= 1
                and cam.shape[1] == 30 and cam.device == dev):
            raise ValueError('cam: expected contiguous CUDA float32 [Rc >= 1, 30]')
        if not (rows.is_cuda and rows.dtype == torch.int32 and rows.is_contiguous() and rows.dim() == 3 and 1 <= rows.shape[0] <= 8
                and rows.shape[1] >= 1 and rows.shape[2] == 3 and rows.device == dev):
            raise ValueError('rows: expected contiguous CUDA int32 [S = 1 .. 8, B, 3] = f0 row | f1 row | cam row')
        if not (candidates.is_cuda and candidates.dtype == torch.float32 and candidates.is_contiguous()
                and candidates.dim() == 1):
            raise ValueError('candidates: expected contiguous CUDA float32 [D]')
        s, b = rows.shape[:2]
        n = len(segments)
        seg_ptr = (ctypes.c_void_p * n)(*[_ptr(t) for t in segments])
        seg_rows = (ctypes.c_int * n)(*[t.shape[0] for t in segments])
        out = torch.empty((b, 1, h, w), dtype=torch.float32, device=dev)
        planes = torch.empty((b, 4, h, w), dtype=torch.float32, device=dev) if stats else None
        index = torch.empty((b, 2, h, w), dtype=torch.int32, device=dev) if stats else None
        code = self._launch('depth_corr_softmax_multi_rows', lambda: self.lib.um_depth_corr_softmax_multi_rows(
            seg_ptr, seg_rows, n, _ptr(cam), cam.shape[0], _ptr(rows), _ptr(candidates), _ptr(out),
            _ptr(planes) if stats else None, _ptr(index) if stats else None, s, b, h, w, 128,
            candidates.numel(), int(bool(from_argmax)), int(peak_radius), _stream()))
        _abi.check(code, 'um_depth_corr_softmax_multi_rows')
        return (out, planes, index) if stats else out
