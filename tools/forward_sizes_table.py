"""The record of the forward-size matrix (tests/forward_sizes.py) on the GPU:

    python tools/forward_sizes_table.py [--out profiles/forward_sizes.txt]

Per row and sample: mean and maximum of |exact-mode prediction - fp64 oracle| next to the fp32 oracle's own (the four figures the gates
of tests/test_forward_sizes_gpu.py compare), then per row the launch-census sides of one forward and the kernels of the encoder's
convolutions as the host mirrors predict and the census of ``_encode`` alone counted them.  Needs an MI355X; the oracle runs on the CPU.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import forward_flags as ff  # noqa: E402
from tests import forward_sizes as fs  # noqa: E402
from tests import test_forward_flags_gpu as flags_gpu  # noqa: E402
from tests import test_forward_sizes_gpu as gpu  # noqa: E402
from unimatch_amd import _abi  # noqa: E402


def encoder_counts(case):
    model = ff.build_model(case).to(gpu.DEV).set_precision('exact')
    assert model.ops is not None
    i0, i1, _ = ff.inputs(case)
    i0, i1 = i0.to(gpu.DEV), i1.to(gpu.DEV)
    with torch.no_grad():
        _, counts = gpu.census(_abi.load(), lambda: model._encode((i0, i1), ff.task_of(case)))
    return {k: counts[k] for k in gpu.CONV_SIDES}


def main():
    out_path = os.path.join(ROOT, 'profiles', 'forward_sizes.txt')
    if '--out' in sys.argv:
        out_path = sys.argv[sys.argv.index('--out') + 1]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = [f'forward-size matrix, exact mode on {torch.cuda.get_device_name(0)} ({cus} CUs): |pred - fp64 oracle| per sample, CONDITIONED weights',
             f'{"row":<24}{"n":>2}{"|truth|":>9}{"gpu mean":>10}{"f32 mean":>10}{"ratio":>7}{"gpu max":>10}{"f32 max":>10}{"ratio":>7}']
    sides, worst = [], (0.0, None)
    for name in fs.RUNNING:
        case = fs.BY_NAME[name]
        preds, counts = gpu.row(name)
        truth = fs.oracle(case, torch.float64)
        for n, (g_mean, g_max, f_mean, f_max) in enumerate(flags_gpu.sample_errors(case, preds[0], fs.answers(case))):
            if g_max > worst[0]:
                worst = (g_max, f'{name}[{n}]')
            lines.append(f'{name:<24}{n:>2}{truth[n].abs().mean().item():>9.3f}{g_mean:>10.2e}{f_mean:>10.2e}'
                         f'{g_mean / max(f_mean, 1e-30):>7.2f}{g_max:>10.2e}{f_max:>10.2e}{g_max / max(f_max, 1e-30):>7.2f}')
        ns = case.ctor['num_scales']
        kinds = fs.encoder_kinds(case.size, ns)
        sides.append(f'{name:<24}sides  ' + ' '.join(f'{k}={v}' for k, v in counts.items() if v and k not in gpu.CONV_SIDES))
        sides.append(f'{"":<24}encoder 64:{kinds[64]} 96:{kinds[96]} 128:{kinds[128]}  predicted {fs.encoder_census(case.size, ns)}'
                     f'  counted {encoder_counts(case)}')
    lines.append(f'largest per-sample max error: {worst[0]:.2e} ({worst[1]}); MAX_FLOOR of the flag matrix, used unchanged: {flags_gpu.MAX_FLOOR:.1e}')
    lines.append('')
    lines.append('launch census of one forward (conv_* left out) and the encoder alone (3x3 stride-1 kernel per width; census of _encode):')
    text = '\n'.join(lines + sides) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
