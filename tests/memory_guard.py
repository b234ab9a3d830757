"""Memory-contract harness: does a call's result depend on memory the call does not own?

``MemoryGuard`` is a context manager that replaces ``torch.empty``, ``torch.empty_like``, ``torch.zeros`` and ``torch.zeros_like``
(the only allocators ``unimatch_amd/*.py`` uses) while it is active.  An allocation on the guarded device becomes the middle of one
``uint8`` block ``[G | nbytes | G]``: both red zones hold ``0xA5``, the payload of an ``empty`` holds the run's fill byte, the payload
of a ``zeros`` holds zero, and the trailing red zone starts at exactly ``nbytes``.  ``place()`` puts a test's input into such a block
(red-zone byte chosen per run).  After the call under test:

* ``check()``            -- every red zone of every block is intact                       (W: no write past a buffer)
* ``inputs_unchanged()`` -- every placed input still holds its bytes                      (I: inputs are read-only)

and ``contract(fn, make_inputs)`` runs ``fn`` under several guards and compares the results' raw bytes:

* across the fill bytes 0xFF / 0x00 / 0x3C                                               (U: nothing unwritten is read)
* across the input red-zone bytes 0xFF / 0x00                                            (R: nothing past an input is read)
* across two runs of one configuration                                                   (base: run-to-run reproducible)

Plain Python: importing it needs no GPU, and with ``device='cpu'`` the whole harness runs on host tensors.  Not for use inside a
graph capture (every allocation launches fills)."""
import os
import sys

import torch

G = 64 * 1024                    # red zone on each side, a multiple of 512: the payload keeps the alignment production tensors have
REDZONE = 0xA5                   # red-zone byte of the product's own allocations
FILLS = (0xFF, 0x00, 0x3C)       # NaN in fp32 / fp16 / bf16 and -1 in counters; zero (what fresh memory tends to hold); finite, plausible
INPUT_REDZONES = (0xFF, 0x00)
PATCHED = ('empty', 'empty_like', 'zeros', 'zeros_like')
_PACKAGE = os.sep + 'unimatch_amd' + os.sep


class ContractViolation(AssertionError):
    """One property of the memory contract failed: ``prop`` is 'W', 'I', 'U', 'R' or 'base'."""

    def __init__(self, prop, message):
        AssertionError.__init__(self, f'[{prop}] {message}')
        self.prop = prop


def _call_site():
    """file:line of the innermost frame inside unimatch_amd (the allocation the product made), else of the harness's caller."""
    f = sys._getframe(2)
    first = None
    while f is not None:
        name = f.f_code.co_filename
        if _PACKAGE in name:
            return f'unimatch_amd{os.sep}{name.split(_PACKAGE)[-1]}:{f.f_lineno}'
        if first is None and os.path.abspath(name) != os.path.abspath(__file__):
            first = f'{os.path.basename(name)}:{f.f_lineno}'
        f = f.f_back
    return first or '?'


class _Block:
    __slots__ = ('block', 'nbytes', 'rz', 'site', 'kind', 'original', 'inout')

    def __init__(self, block, nbytes, rz, site, kind):
        self.block, self.nbytes, self.rz, self.site, self.kind = block, nbytes, rz, site, kind
        self.original = None     # placed inputs: the bytes they were given (host copy)
        self.inout = False       # placed and declared as written by the call (a state updated in place): exempt from I, not from W

    def payload(self):
        return self.block[G:G + self.nbytes]


class MemoryGuard:
    def __init__(self, device='cuda', fill=0xFF, input_redzone=0xFF):
        self.device = self._canonical(torch.device(device))
        self.fill, self.input_redzone = int(fill), int(input_redzone)
        self.blocks = []
        self.passed_through = []         # call sites of allocations ON the guarded device that the wrappers did not understand
        self._saved = None

    # ------------------------------------------------------------------ context
    def __enter__(self):
        if self._saved is not None:
            raise RuntimeError('MemoryGuard is not re-entrant')
        self._saved = {name: getattr(torch, name) for name in PATCHED}
        torch.empty = self._wrap_new('empty')
        torch.zeros = self._wrap_new('zeros')
        torch.empty_like = self._wrap_like('empty')
        torch.zeros_like = self._wrap_like('zeros')
        return self

    def __exit__(self, *exc):
        for name, fn in self._saved.items():
            setattr(torch, name, fn)
        self._saved = None
        return False

    # ------------------------------------------------------------------ allocation
    @staticmethod
    def _canonical(dev):
        if dev.type == 'cuda' and dev.index is None:
            return torch.device('cuda', torch.cuda.current_device())
        return torch.device(dev.type) if dev.type == 'cpu' else dev

    def _guarded(self, shape, dtype, kind, payload_byte, rz, site):
        numel = 1
        for s in shape:
            numel *= int(s)
        nbytes = numel * dtype.itemsize
        block = self._saved['empty'](G + nbytes + G, dtype=torch.uint8, device=self.device)      # (inside the context only)
        block[:G].fill_(rz)
        block[G + nbytes:].fill_(rz)
        if payload_byte is not None and nbytes:
            block[G:G + nbytes].fill_(payload_byte)
        rec = _Block(block, nbytes, rz, site, kind)
        self.blocks.append(rec)
        return rec, block[G:G + nbytes].view(dtype).view(tuple(int(s) for s in shape))

    def _pass(self, original, args, kwargs):
        """The untouched call; one that still lands on the guarded device is counted, so a test can insist on none."""
        out = original(*args, **kwargs)
        if isinstance(out, torch.Tensor) and self._canonical(out.device) == self.device:
            self.passed_through.append(_call_site())
        return out

    @staticmethod
    def _size(args):
        if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
            args = tuple(args[0])
        if all(isinstance(s, int) and not isinstance(s, bool) and s >= 0 for s in args):
            return tuple(args)
        return None

    def _wrap_new(self, kind):
        original = self._saved[kind]

        def alloc(*args, **kwargs):
            if set(kwargs) - {'dtype', 'device'}:
                return self._pass(original, args, kwargs)
            try:
                dev = self._canonical(torch.device(kwargs['device']) if kwargs.get('device') is not None else torch.get_default_device())
            except (TypeError, RuntimeError):
                return self._pass(original, args, kwargs)
            shape = self._size(args)
            dtype = kwargs.get('dtype') or torch.get_default_dtype()
            if dev != self.device or shape is None or not isinstance(dtype, torch.dtype) or dtype.is_complex:
                return self._pass(original, args, kwargs)
            return self._guarded(shape, dtype, kind, self.fill if kind == 'empty' else 0, REDZONE, _call_site())[1]
        alloc.__name__ = kind
        return alloc

    def _wrap_like(self, kind):
        original = self._saved[kind + '_like']

        def alloc_like(*args, **kwargs):
            t = args[0] if len(args) == 1 else None
            if (not isinstance(t, torch.Tensor) or set(kwargs) - {'dtype', 'device'} or not t.is_contiguous() or t.dtype.is_complex
                    or t.layout != torch.strided):
                return self._pass(original, args, kwargs)
            try:
                dev = self._canonical(torch.device(kwargs['device']) if kwargs.get('device') is not None else t.device)
            except (TypeError, RuntimeError):
                return self._pass(original, args, kwargs)
            dtype = kwargs.get('dtype') or t.dtype
            if dev != self.device or not isinstance(dtype, torch.dtype):
                return self._pass(original, args, kwargs)
            return self._guarded(tuple(t.shape), dtype, kind, self.fill if kind == 'empty' else 0, REDZONE, _call_site())[1]
        alloc_like.__name__ = kind + '_like'
        return alloc_like

    def place(self, t, inout=False):
        """A copy of ``t`` (any device) on the guarded device, inside a block whose red zones hold this run's input byte."""
        t = t.detach().contiguous()
        rec, view = self._guarded(tuple(t.shape), t.dtype, 'input', None, self.input_redzone, _call_site())
        view.copy_(t)
        rec.original = t.cpu().reshape(-1).view(torch.uint8).clone() if t.numel() else torch.zeros(0, dtype=torch.uint8)
        rec.inout = bool(inout)
        return view

    def place_module(self, module):
        """Move every parameter and buffer of an ``nn.Module`` into placed blocks (in place); returns the module."""
        for p in list(module.parameters()) + list(module.buffers()):
            p.data = self.place(p.data)
        return module

    # ------------------------------------------------------------------ verdicts
    def _sync(self):
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)

    def check(self):
        """W: every red zone of every live block holds its byte.  Names the allocation (call site) and where the damage starts."""
        self._sync()
        if not self.blocks:
            return
        flags = torch.stack([torch.stack([(b.block[:G] != b.rz).any(), (b.block[G + b.nbytes:] != b.rz).any()]) for b in self.blocks])
        if not bool(flags.any()):
            return
        flags = flags.cpu()
        msgs = []
        for b, (lead, trail) in zip(self.blocks, flags.tolist()):
            if lead:
                bad = (b.block[:G] != b.rz).nonzero().flatten()
                msgs.append(f'{b.kind} of {b.nbytes} bytes allocated at {b.site}: {bad.numel()} damaged bytes BEFORE the payload, the '
                            f'nearest {G - int(bad[-1])} bytes before its first byte')
            if trail:
                bad = (b.block[G + b.nbytes:] != b.rz).nonzero().flatten()
                msgs.append(f'{b.kind} of {b.nbytes} bytes allocated at {b.site}: {bad.numel()} damaged bytes AFTER the payload, the '
                            f'first {int(bad[0])} bytes past its end')
        raise ContractViolation('W', 'red zone damaged: ' + '; '.join(msgs[:8]))

    def inputs_unchanged(self):
        """I: every placed input still holds the bytes it was given."""
        self._sync()
        for b in self.blocks:
            if b.original is None or b.inout:
                continue
            now = b.payload().cpu()
            if not torch.equal(now, b.original):
                first = int((now != b.original).nonzero()[0])
                raise ContractViolation('I', f'the input of {b.nbytes} bytes placed at {b.site} was written: first changed byte at offset {first}')


# ---------------------------------------------------------------------- the driver
def raw_bytes(x):
    """The comparable form of a result: tensors as host uint8 vectors, containers member by member, everything else as it is."""
    if isinstance(x, torch.Tensor):
        t = x.detach().contiguous()
        return t.cpu().reshape(-1).view(torch.uint8) if t.numel() else torch.zeros(0, dtype=torch.uint8)
    if isinstance(x, (tuple, list)):
        return tuple(raw_bytes(v) for v in x)
    if isinstance(x, dict):
        return {k: raw_bytes(v) for k, v in x.items()}
    return x


def _differences(a, b, path='result'):
    if isinstance(a, torch.Tensor):
        if not isinstance(b, torch.Tensor) or a.shape != b.shape:
            return [f'{path}: sizes differ']
        if torch.equal(a, b):
            return []
        bad = (a != b).nonzero().flatten()
        return [f'{path}: {bad.numel()} of {a.numel()} bytes differ, the first at byte {int(bad[0])}, the last at byte {int(bad[-1])}']
    if isinstance(a, tuple):
        if not isinstance(b, tuple) or len(a) != len(b):
            return [f'{path}: lengths differ']
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in _differences(x, y, f'{path}[{i}]')]
    if isinstance(a, dict):
        if not isinstance(b, dict) or set(a) != set(b):
            return [f'{path}: keys differ']
        return [d for k in a for d in _differences(a[k], b[k], f'{path}[{k!r}]')]
    return [] if a == b else [f'{path}: {a!r} != {b!r}']


def contract(fn, make_inputs, device='cuda', make_ops=None, mask=None):
    """Run ``fn(ops, *make_inputs(guard))`` once per configuration and assert W, I, U, R and run-to-run reproducibility.

    ``make_inputs(guard)`` builds the call's arguments (deterministically) and puts every tensor the call reads through
    ``guard.place``; ``make_ops()`` returns a FRESH ops object per run (a cached weight plane or workspace of run 1 would keep run 1's
    fill in run 2); ``mask(raw result)`` blanks regions that are unspecified by contract before the comparison (the caller's
    DONT_CARE table).  Returns the raw result of the first run; ``contract.last_sites`` lists the call sites of the last run's guarded
    allocations and ``contract.last_passed_through`` those of allocations on the guarded device that the wrappers let through untouched
    (a test can assert that the product's allocations really went through the guard, all of them)."""
    configs = [('first', FILLS[0], INPUT_REDZONES[0]), ('repeat', FILLS[0], INPUT_REDZONES[0])]
    configs += [('fill', f, INPUT_REDZONES[0]) for f in FILLS[1:]] + [('redzone', FILLS[0], r) for r in INPUT_REDZONES[1:]]
    first = None
    for what, fill, rz in configs:
        ops = make_ops() if make_ops is not None else None
        with MemoryGuard(device, fill=fill, input_redzone=rz) as guard:
            args = make_inputs(guard)
            out = fn(ops, *args)
            guard.check()
            guard.inputs_unchanged()
            got = raw_bytes(out)
            contract.last_sites = [b.site for b in guard.blocks if b.kind != 'input']
            contract.last_passed_through = list(guard.passed_through)
        del out, args, ops
        if mask is not None:
            got = mask(got)
        if first is None:
            first = got
            continue
        diff = _differences(first, got)
        if diff:
            prop = {'repeat': 'base', 'fill': 'U', 'redzone': 'R'}[what]
            detail = {'repeat': 'two runs of one configuration differ',
                      'fill': f'the result changes when fresh memory holds 0x{fill:02X} instead of 0x{FILLS[0]:02X}',
                      'redzone': f'the result changes when the bytes around the inputs are 0x{rz:02X} instead of 0x{INPUT_REDZONES[0]:02X}'}[what]
            raise ContractViolation(prop, detail + ': ' + '; '.join(diff[:6]))
    return first


contract.last_sites = []
contract.last_passed_through = []
