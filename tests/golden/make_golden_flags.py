"""Mint the forward-flag fixtures from the REAL reference (runs only where the reference checkout exists):

    python tests/golden/make_golden_flags.py

For every case of ``tests/forward_flags.py`` the reference's ``UniMatch.forward`` runs in fp32 on the case's seeded weights and inputs.
Stored per case: ``<name>.fp32`` (the prediction at 8 threads) and ``<name>.spread`` (the scalar ``mean|8 threads - 1 thread|``: the
reference's own noise between two summation orders, the unit of the oracle-vs-reference gate); for a case the reference cannot run,
``<name>.raises`` (the exception's class name).  Arrays only.  The cases name their fixture (``flags``, ``flags_bidir``, ``flags_b2``):
three files, so that each stays a small one.  The archives are written with a fixed timestamp: running this again reproduces them
byte for byte.
"""
import os
import sys
import warnings
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get('UNIMATCH_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, REFERENCE)
warnings.filterwarnings('ignore')

from unimatch.unimatch import UniMatch as RefUniMatch  # noqa: E402

from tests import forward_flags as ff  # noqa: E402


def run_reference(case, threads):
    model = RefUniMatch(**case.ctor).eval()
    model.load_state_dict(ff.state_dict(case))
    i0, i1, cam = ff.inputs(case)
    torch.set_num_threads(threads)
    with torch.no_grad():
        out = model(i0, i1, **case.fwd, **cam)['flow_preds']
    assert len(out) == 1
    return out[0]


def save(name, arrays):
    """``np.savez_compressed`` with every member stamped 1980-01-01: the same arrays give the same bytes."""
    path = os.path.join(HERE, name + '.npz')
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, 'w') as f:
                np.lib.format.write_array(f, np.asarray(arrays[key]), allow_pickle=False)
    print(f'{name}.npz  {os.path.getsize(path) / 1024:.0f} KiB')


def main():
    out = {}
    for case in ff.CASES:
        arrays = out.setdefault(case.fixture, {})
        try:
            o8 = run_reference(case, 8)
        except Exception as e:                                    # noqa: BLE001 -- which exception is what gets recorded
            assert case.raises is not None, (case.name, e)
            arrays[f'{case.name}.raises'] = np.array(type(e).__name__)
            print(f'  {case.name}: raises {type(e).__name__}: {str(e)[:90]}')
            continue
        assert case.raises is None, case.name
        o1 = run_reference(case, 1)
        spread = (o8 - o1).abs().mean().item()
        arrays[f'{case.name}.fp32'] = o8.numpy()
        arrays[f'{case.name}.spread'] = np.array(spread, dtype=np.float64)
        print(f'  {case.name}: out {tuple(o8.shape)} |out| mean {o8.abs().mean():.3f}  8thr-vs-1thr mean {spread:.2e}')
    for name, arrays in out.items():
        save(name, arrays)


if __name__ == '__main__':
    main()
