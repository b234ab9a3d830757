"""Shared by the CPU and GPU tests of ``unimatch_amd.visualize``: the fixtures of tests/golden/visualize.npz (minted from the
reference by tests/golden/make_golden_visualize.py) and the inverse of the plasma table."""
import os

import numpy as np

from unimatch_amd import visualize

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'visualize.npz')
GROUPS = 4
_cache = {}


def load_golden():
    if 'g' not in _cache:
        _cache['g'] = dict(np.load(GOLDEN))
    return _cache['g']


def plasma_index(rgb):
    """``rgb [..., 3]`` uint8 of plasma colours -> the table index of each (the 256 colours are distinct)."""
    table = visualize.colormap('plasma').astype(np.int64)
    code = (table[:, 0] << 16) | (table[:, 1] << 8) | table[:, 2]
    assert len(set(code.tolist())) == 256
    order = np.argsort(code)
    c = rgb.astype(np.int64)
    c = (c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2]
    pos = np.searchsorted(code[order], c)
    assert np.array_equal(code[order][np.clip(pos, 0, 255)], c), 'a colour that is not in the plasma table'
    return order[pos]
