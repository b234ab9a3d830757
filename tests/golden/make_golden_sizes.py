"""Mint the forward-size fixtures from the REAL reference (runs only where the reference checkout exists):

    python tests/golden/make_golden_sizes.py

The recipe of ``make_golden_flags.py`` (its ``run_reference`` and ``save`` are used as they are) over the rows of
``tests/forward_sizes.py``: per row ``<name>.fp32`` (the reference's fp32 prediction at 8 threads) and ``<name>.spread`` (the scalar
``mean|8 threads - 1 thread|``, the unit of the oracle-vs-reference gate).  Arrays only.  The rows name their fixture (``sizes_a`` ..
``sizes_d``) so that each file stays a small one; the archives carry a fixed timestamp, so running this again reproduces them byte
for byte.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_flags as flags  # noqa: E402  (puts the repository and the reference on sys.path)

from tests import forward_sizes as fs  # noqa: E402


def main():
    out = {}
    for case in fs.CASES:
        assert case.raises is None, case.name                     # every row of this matrix runs in the reference
        o8, o1 = flags.run_reference(case, 8), flags.run_reference(case, 1)
        spread = (o8 - o1).abs().mean().item()
        arrays = out.setdefault(case.fixture, {})
        arrays[f'{case.name}.fp32'] = o8.numpy()
        arrays[f'{case.name}.spread'] = np.array(spread, dtype=np.float64)
        print(f'  {case.name}: out {tuple(o8.shape)} |out| mean {o8.abs().mean():.3f}  8thr-vs-1thr mean {spread:.2e}')
    for name in sorted(out):
        flags.save(name, out[name])


if __name__ == '__main__':
    main()
