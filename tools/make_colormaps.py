"""Generate ``unimatch_amd/colormaps.json``: the two 256 x 3 uint8 tables of ``unimatch_amd.visualize``, from matplotlib's listed
colormap data (run where matplotlib is installed; the package itself never imports it):

    python tools/make_colormaps.py [--check]

  plasma   ``floor(c * 255)``: what ``(ScalarMappable(cmap='plasma').to_rgba(x)[:, :, :3] * 255).astype(np.uint8)`` gives for each of
           the 256 entries (asserted below, together with the 256 colours being distinct, which the tests rely on to map a colour
           back to its index).
  inferno  ``rint(c * 255)``, on the assumption that OpenCV rounds when it builds ``COLORMAP_INFERNO`` from the same data.  OpenCV
           was not available where this was written, so equality with its table is unverified.  Stored R, G, B.

``--check`` compares the committed file with a fresh table instead of writing it.
"""
import json
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'unimatch_amd', 'colormaps.json')


def tables():
    import matplotlib
    from matplotlib import cm
    from matplotlib._cm_listed import _inferno_data, _plasma_data
    plasma = np.floor(np.asarray(_plasma_data, dtype=np.float64) * 255).astype(np.uint8)
    inferno = np.rint(np.asarray(_inferno_data, dtype=np.float64) * 255).astype(np.uint8)
    assert plasma.shape == inferno.shape == (256, 3)
    # the reference's expression, entry by entry: values at the bin centres (i + 0.5) / 256 land in entry i
    x = ((np.arange(256) + 0.5) / 256).astype(np.float32).reshape(1, 256)
    mapper = cm.ScalarMappable(norm=matplotlib.colors.Normalize(vmin=0.0, vmax=1.0), cmap='plasma')
    ref = (mapper.to_rgba(x)[:, :, :3] * 255).astype(np.uint8)[0]
    assert np.array_equal(ref, plasma), 'plasma: floor(c * 255) is not what ScalarMappable gives'
    assert len({tuple(c) for c in plasma.tolist()}) == 256, 'plasma: colours are not distinct'
    return {'matplotlib_version': matplotlib.__version__, 'plasma': plasma.tolist(), 'inferno': inferno.tolist()}


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    new = tables()
    if '--check' in argv:
        with open(OUT) as f:
            old = json.load(f)
        same = all(old[k] == new[k] for k in ('plasma', 'inferno'))
        print('colormaps.json', 'matches' if same else 'DIFFERS from', f"matplotlib {new['matplotlib_version']}")
        return 0 if same else 1
    with open(OUT, 'w') as f:
        f.write('{"matplotlib_version": %s,\n' % json.dumps(new['matplotlib_version']))
        for k in ('plasma', 'inferno'):
            f.write(' "%s": [\n' % k)
            rows = new[k]
            for i in range(0, 256, 8):
                f.write('  ' + ', '.join(json.dumps(r, separators=(',', ':')) for r in rows[i:i + 8]) + (',\n' if i < 248 else '\n'))
            f.write(' ]%s\n' % (',' if k == 'plasma' else ''))
        f.write('}\n')
    print('wrote', OUT)
    return 0


if __name__ == '__main__':
    sys.exit(main())
