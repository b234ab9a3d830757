"""profiles/degenerate_content.txt from the output of the degenerate-content GPU tests.

    python -m pytest tests/test_degenerate_content_gpu.py -s -q > LOG
    python tools/degenerate_content_table.py LOG [MACHINE] > profiles/degenerate_content.txt

The tests print one ``DC|row|item|measured|reference-side figure|bound`` line per gate (tests/test_degenerate_content_gpu.py: ``record``),
the matching-statistics gates print tests/test_match_stats_gpu.py's own line, and the forwards print ``check_gates``' line:
``case kind [gpu mean, gpu max | fp32 oracle mean, fp32 oracle max]`` per sample."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.degenerate_content import KINDS  # noqa: E402
from tests.test_forward_flags_gpu import MAX_FLOOR  # noqa: E402


def main(path, machine='AMD Instinct MI355X (gfx950)'):
    rows, stats, forwards = [], [], []
    for line in open(path):
        line = line.strip().lstrip('.')
        if line.startswith('DC|'):
            rows.append(line.split('|')[1:])
        elif line.startswith('duplicated ('):
            stats.append(line)
        elif re.match(r'^(flow|stereo|depth)_s\d\w* (%s) .*\[' % '|'.join(KINDS), line):
            forwards.append(line)
    print(f'degenerate content, exact mode on {machine}: max |kernel - fp64| per gate')
    print('reference: for P3 / P4 and offset rows max |fp32 torch - fp64| on the same tensor (bound = 2 x that + the tolerance); otherwise the')
    print('tolerance of the entry point\'s own test times max(1, |want|max), which is then also the bound')
    print()
    print(f'{"row":78s} {"item":22s} {"measured":>10s} {"reference":>10s} {"bound":>10s}')
    for r in rows:
        r = r + [''] * (5 - len(r))
        print(f'{r[0]:78s} {r[1]:22s} {r[2]:>10s} {r[3]:>10s} {r[4]:>10s}')
    print()
    print('matching statistics on duplicated keys (the gates of tests/test_match_stats_gpu.py)')
    for s in stats:
        print(s)
    print()
    print(f'whole forwards: case kind [gpu mean, gpu max | fp32 oracle mean, fp32 oracle max] per sample; gates mean <= 3 x + 1e-4, max <= 3 x + {MAX_FLOOR:.0e}')
    for f in forwards:
        print(f)


if __name__ == '__main__':
    main(*sys.argv[1:3])
