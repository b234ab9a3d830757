"""Mint ``match_stats.npz`` from the REAL reference (runs only where the reference checkout exists):

    UNIMATCH_REFERENCE=<checkout> python tests/golden/make_golden_match_stats.py

Pins the matching distribution ``prob`` that the reference's matching layer returns next to the flow and that
``unimatch_amd.confidence`` takes its statistics from (``unimatch/matching.py``):

  * ``global_correlation_softmax`` on seeded features, B = 2 at 6 x 10, with and without ``pred_bidir_flow``: the call without it
    returns the first half of the call with it bit for bit (asserted here), so only the bidirectional ``prob`` is stored;
  * ``global_correlation_softmax_stereo`` on seeded features, B = 2 at 4 x 12.

The reference functions take any channel count; 32 channels keep the file at tens of KB.

The second view is a permuted, noisy copy of the first with a per-token gain, so that the rows run from flat to peaked.  The features
are stored as float16 (the values the reference was run on, exactly) and the returned ``prob`` as float32.  Only inputs and recorded
results are stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get('UNIMATCH_REFERENCE')
if not REFERENCE or not os.path.isdir(REFERENCE):
    raise SystemExit('set UNIMATCH_REFERENCE to a checkout of the reference')
sys.path.insert(0, REFERENCE)

from unimatch.matching import global_correlation_softmax, global_correlation_softmax_stereo  # noqa: E402


def features(seed, b, h, w, c=32, stereo=False):
    g = torch.Generator().manual_seed(seed)
    f0 = torch.randn(b, c, h, w, generator=g)
    if stereo:                                                            # the match lies to the left: shift every scanline
        src = f0.roll(2, dims=-1)
    else:
        perm = torch.stack([torch.randperm(h * w, generator=g) for _ in range(b)])
        src = f0.flatten(2).gather(2, perm[:, None].expand(b, c, h * w)).view(b, c, h, w)
    gain = torch.rand(b, 1, h, w, generator=g) * 1.6                      # 0: a flat row ... 1.6: a sharp peak
    f1 = gain * src + 0.5 * torch.randn(b, c, h, w, generator=g)
    return f0.half().float(), f1.half().float()


def main():
    out = {}
    f0, f1 = features(71, 2, 6, 10)
    out['flow_f0'], out['flow_f1'] = f0.half().numpy(), f1.half().numpy()
    out['flow_prob_bidir'] = global_correlation_softmax(f0, f1, pred_bidir_flow=True)[1].numpy()
    assert np.array_equal(global_correlation_softmax(f0, f1, pred_bidir_flow=False)[1].numpy(), out['flow_prob_bidir'][:2])
    s0, s1 = features(72, 2, 4, 12, stereo=True)
    out['stereo_f0'], out['stereo_f1'] = s0.half().numpy(), s1.half().numpy()
    out['stereo_prob'] = global_correlation_softmax_stereo(s0, s1)[1].numpy()
    path = os.path.join(HERE, 'match_stats.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
