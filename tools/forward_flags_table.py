"""The error table of the forward-flag matrix (tests/forward_flags.py) on the GPU:

    python tools/forward_flags_table.py [--out profiles/forward_flags.txt]

Per case and sample: mean and maximum of |exact-mode prediction - fp64 oracle| next to the fp32 oracle's own, and their ratios; for the
arg-max depth case also the share of pixels further than 1e-3.  The last line is the largest per-sample maximum error, the figure
``MAX_FLOOR`` of tests/test_forward_flags_gpu.py is derived from (4 x, capped at 1e-3).  Needs an MI355X; the oracle runs on the CPU.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import forward_flags as ff  # noqa: E402
from tests import test_forward_flags_gpu as gpu  # noqa: E402


def main():
    out_path = os.path.join(ROOT, 'profiles', 'forward_flags.txt')
    if '--out' in sys.argv:
        out_path = sys.argv[sys.argv.index('--out') + 1]
    lines = [f'forward-flag matrix, exact mode on {torch.cuda.get_device_name(0)}: |pred - fp64 oracle| per sample, CONDITIONED weights',
             f'{"case":<20}{"n":>2}{"|truth|":>9}{"gpu mean":>10}{"f32 mean":>10}{"ratio":>7}{"gpu max":>10}{"f32 max":>10}{"ratio":>7}  note']
    worst = (0.0, None)
    for name in ff.RUNNING:
        case = ff.BY_NAME[name]
        for parts in ((1, 2) if case.batch > 1 else (1,)):
            pred = gpu.run_gpu(case, parts=parts, calls=parts)[0][-1]
            truth = ff.oracle(case, torch.float64)
            for n, (g_mean, g_max, f_mean, f_max) in enumerate(gpu.sample_errors(case, pred)):
                note = 'two parts' if parts > 1 else ''
                if case.fwd.get('depth_from_argmax'):
                    far = ((pred[n].double() - truth[n]).abs() > gpu.ARGMAX_TOL).float().mean().item()
                    note = f'arg-max: {100 * far:.3f} % of pixels beyond {gpu.ARGMAX_TOL:g} (not part of the floor)'
                elif g_max > worst[0]:
                    worst = (g_max, f'{name}[{n}]')
                lines.append(f'{name:<20}{n:>2}{truth[n].abs().mean().item():>9.3f}{g_mean:>10.2e}{f_mean:>10.2e}'
                             f'{g_mean / max(f_mean, 1e-30):>7.2f}{g_max:>10.2e}{f_max:>10.2e}{g_max / max(f_max, 1e-30):>7.2f}  {note}')
    lines.append(f'largest per-sample max error: {worst[0]:.2e} ({worst[1]})  ->  MAX_FLOOR = 4 x = {min(4 * worst[0], 1e-3):.1e}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
