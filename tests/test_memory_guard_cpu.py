"""The memory-contract harness (tests/memory_guard.py) must be able to fail: plain-torch stand-ins for a kernel, each with one
injected defect, run on host tensors; every defect has to fail exactly the property it targets.  The same stand-ins run once on the
device in tests/test_memory_contract_gpu.py."""
import glob
import os
import re

import pytest
import torch

from tests import memory_guard as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------- stand-ins for a kernel (shared with the device self-checks)
def make_standin_inputs(device):
    def make(guard):
        x = torch.arange(6 * 5, dtype=torch.float32).view(6, 5) / 7.0
        return (guard.place(x),)
    return make


def _bytes_with_slack(t, before, after):
    """The bytes of ``t`` plus ``before`` / ``after`` bytes around them -- inside the guarded block the tensor lives in."""
    flat = t.view(-1).view(torch.uint8)
    return torch.as_strided(flat, (before + flat.numel() + after,), (1,), flat.storage_offset() - before)


def standin_good(device):
    def fn(ops, x):
        out = torch.empty(x.shape, dtype=torch.float32, device=device)
        tmp = torch.zeros_like(x)
        tmp += x
        out.copy_(tmp * 2)
        return out, torch.empty_like(x).copy_(x + 1)
    return fn


def standin_writes_past(device):
    def fn(ops, x):
        out = torch.empty(x.shape, dtype=torch.float32, device=device)
        out.copy_(x * 2)
        _bytes_with_slack(out, 0, 1)[-1] = 7
        return out
    return fn


def standin_writes_before(device):
    def fn(ops, x):
        out = torch.empty(x.shape, dtype=torch.float32, device=device)
        out.copy_(x * 2)
        _bytes_with_slack(out, 1, 0)[0] = 7
        return out
    return fn


def standin_leaves_a_row(device):
    def fn(ops, x):
        out = torch.empty(x.shape, dtype=torch.float32, device=device)
        out[:-1].copy_(x[:-1] * 2)
        return out
    return fn


def standin_reads_past_input(device):
    def fn(ops, x):
        out = torch.empty(x.shape, dtype=torch.float32, device=device)
        wide = torch.as_strided(x, (x.numel() + 1,), (1,), x.storage_offset())          # one element past the input
        out.copy_(x * 2)
        out[-1, -1] = wide[-1:].view(torch.uint8).float().sum()                          # finite, and depends on those four bytes
        return out
    return fn


def standin_writes_its_input(device):
    def fn(ops, x):
        out = torch.empty(x.shape, dtype=torch.float32, device=device)
        out.copy_(x * 2)
        x[2, 3] += 1.0
        return out
    return fn


DEFECTS = [(standin_writes_past, 'W', 'AFTER the payload, the first 0 bytes past'), (standin_writes_before, 'W', 'BEFORE the payload, the nearest 1 bytes'),
           (standin_leaves_a_row, 'U', None), (standin_reads_past_input, 'R', None), (standin_writes_its_input, 'I', None)]


def test_a_correct_stand_in_passes():
    got = mg.contract(standin_good('cpu'), make_standin_inputs('cpu'), device='cpu')
    want = (torch.arange(30, dtype=torch.float32) / 7.0)
    assert torch.equal(got[0].view(torch.float32), want * 2) and torch.equal(got[1].view(torch.float32), want + 1)


@pytest.mark.parametrize('defect,prop,text', DEFECTS, ids=[d[0].__name__ for d in DEFECTS])
def test_each_defect_fails_the_property_it_targets(defect, prop, text):
    with pytest.raises(mg.ContractViolation) as exc:
        mg.contract(defect('cpu'), make_standin_inputs('cpu'), device='cpu')
    assert exc.value.prop == prop, str(exc.value)
    if text:
        assert text in str(exc.value), str(exc.value)
    if prop == 'W':                                       # the damaged allocation is named by its call site
        assert re.search(r'test_memory_guard_cpu\.py:\d+', str(exc.value)), str(exc.value)


def test_the_call_site_inside_the_package_is_named():
    """An allocation made by unimatch_amd code is reported as unimatch_amd/<file>:<line>, not as the test's line."""
    from unimatch_amd.ops import WorkspaceRegistry
    reg = WorkspaceRegistry(stream=lambda: 0, capturing=lambda: False)
    with mg.MemoryGuard('cpu') as guard:
        buf = reg._workspace('attn_ksplit', (1, 2), 300, torch.device('cpu'), 8)
        assert buf.numel() == 300 and not buf.any()
        _bytes_with_slack(buf, 0, 3)[-1] = 1
        with pytest.raises(mg.ContractViolation, match=r'zeros of 300 bytes allocated at unimatch_amd.ops\.py:\d+: 1 damaged bytes AFTER the '
                                                       r'payload, the first 2 bytes past') as exc:
            guard.check()
    assert exc.value.prop == 'W'


def test_block_layout():
    """[G | nbytes | G] in one uint8 block: red zones 0xA5, payload = fill byte (empty) or zero (zeros), the trailing red zone starts at
    exactly nbytes (no rounding), placed inputs carry the run's input byte, every block is kept."""
    with mg.MemoryGuard('cpu', fill=0x3C, input_redzone=0x00) as guard:
        e = torch.empty((3, 7), dtype=torch.float16, device='cpu')
        z = torch.zeros(5, dtype=torch.int32, device='cpu')
        el = torch.empty_like(e)
        zl = torch.zeros_like(e, dtype=torch.float32)
        p = guard.place(torch.full((3,), 2.0))
        n0 = torch.empty(0, dtype=torch.uint8, device='cpu')
    assert mg.G == 65536 and mg.G % 512 == 0
    assert [b.nbytes for b in guard.blocks] == [42, 20, 42, 84, 12, 0]
    assert [b.kind for b in guard.blocks] == ['empty', 'zeros', 'empty', 'zeros', 'input', 'empty']
    for b, t in zip(guard.blocks, (e, z, el, zl, p, n0)):
        assert b.block.dtype == torch.uint8 and b.block.numel() == 2 * mg.G + b.nbytes
        assert t.data_ptr() == b.block.data_ptr() + mg.G or b.nbytes == 0
        rz = 0x00 if b.kind == 'input' else 0xA5
        assert (b.block[:mg.G] == rz).all() and (b.block[mg.G + b.nbytes:] == rz).all()
    assert e.shape == (3, 7) and e.dtype == torch.float16 and (e.view(torch.uint8) == 0x3C).all() and (el.view(torch.uint8) == 0x3C).all()
    assert z.dtype == torch.int32 and not z.any() and zl.dtype == torch.float32 and zl.shape == (3, 7) and not zl.any()
    assert torch.equal(p, torch.full((3,), 2.0))
    guard.check()
    guard.inputs_unchanged()


def test_context_restores_the_four_functions():
    before = [getattr(torch, n) for n in mg.PATCHED]
    with mg.MemoryGuard('cpu'):
        assert all(getattr(torch, n) is not f for n, f in zip(mg.PATCHED, before))
    assert [getattr(torch, n) for n in mg.PATCHED] == before
    with pytest.raises(KeyError):
        with mg.MemoryGuard('cpu'):
            raise KeyError('from the body')
    assert [getattr(torch, n) for n in mg.PATCHED] == before


def test_pass_through_cases_stay_untouched():
    with mg.MemoryGuard('cpu') as guard:
        other = torch.empty(4, device='meta')                                      # another device
        dest = torch.arange(4.0)
        into = torch.zeros(4, out=dest)                                            # out=
        pinned = torch.empty(4, device='cpu', requires_grad=True)                  # a keyword the wrapper does not know
        strided = torch.empty_like(torch.arange(6.0).view(2, 3).t())               # not contiguous: layout questions stay torch's
        fmt = torch.zeros_like(dest, memory_format=torch.contiguous_format)
        sym = torch.empty(torch.Size([2, 2]), device='cpu')                        # understood: a Size
        assert len(guard.blocks) == 1 and sym.shape == (2, 2)
        assert len(guard.passed_through) == 4                                      # ... and counted when they land on the guarded device
    assert other.device.type == 'meta' and into is dest and not dest.any() and pinned.requires_grad
    assert strided.shape == (3, 2) and fmt.shape == (4,)
    with mg.MemoryGuard('meta') as guard:                                          # the target device is a parameter
        torch.empty(4, device='cpu')
        assert not guard.blocks


# ---------------------------------------------------------------------- the package allocates through the four wrapped functions only
RAW_IDIOMS = re.compile(r'\b(empty_strided|empty_permuted|empty_quantized|new_empty|new_empty_strided|resize_|resize_as_|set_|UntypedStorage|'
                        r'TypedStorage|caching_allocator_alloc|FloatTensor|HalfTensor|ByteTensor|IntTensor|DoubleTensor|LongTensor)\s*\(|'
                        r'\btorch\.Tensor\s*\(|\.new\s*\(')
VALUE_IDIOMS = re.compile(r'\b(new_zeros|new_ones|new_full|new_tensor)\s*\(')
# value-constructing allocations outside ops.py that the harness does not wrap: {file: count}; each is consumed by torch, not handed to
# a kernel as scratch (refine_nhwc.py: channel padding that goes through torch.cat)
KNOWN_VALUE_SITES = {'refine_nhwc.py': 1}


def test_package_allocates_device_memory_through_the_wrapped_functions_only():
    """Memory that a kernel writes or finds zeroed comes from torch.empty / empty_like / zeros / zeros_like: no other idiom for raw
    memory anywhere in unimatch_amd/*.py, none of the new_* family outside the listed sites, and ops.py -- where every kernel's
    outputs and scratch are allocated -- uses nothing else at all (ones / full / arange there would be a new idiom to wrap)."""
    files = sorted(glob.glob(os.path.join(ROOT, 'unimatch_amd', '*.py')))
    assert len(files) > 10
    value_sites = {}
    for path in files:
        text = open(path).read()
        name = os.path.basename(path)
        assert not RAW_IDIOMS.search(text), (name, RAW_IDIOMS.search(text).group(0))
        if VALUE_IDIOMS.search(text):
            value_sites[name] = len(VALUE_IDIOMS.findall(text))
    assert value_sites == KNOWN_VALUE_SITES
    ops = open(os.path.join(ROOT, 'unimatch_amd', 'ops.py')).read()
    factories = set(re.findall(r'\btorch\.(empty\w*|zeros\w*|ones\w*|full\w*|rand\w*|arange|eye|linspace|tensor|as_tensor)\s*\(', ops))
    assert factories <= set(mg.PATCHED) | {'arange'}, factories                  # arange: pack_kv4_weights' index permutation, host logic
    assert len(re.findall(r'\btorch\.(?:empty|empty_like)\s*\(', ops)) >= 60      # ... and the harness sees the sites it was written for
