"""Shared by test_metrics_cpu.py and test_metrics_gpu.py: the fixture, the two comparison rules, seeded inputs.

Comparison rules (tests/golden/metrics.npz holds results recorded from the reference):

  share   1px / 3px / 5px / f1 / d1 / thres* / bad / a1..a3 are ``count / n`` with exact counts: the reference's value is that quotient
          rounded once in its dtype (f1: times 100, one more rounding), so the two agree to one spacing of the recorded dtype.
  sum     EPE, speed bins, matched / unmatched, abs_rel, sq_rel, rmse, rmse_log: the reference pools float32 values with float32
          pairwise summation, forward error ~ log2(n) 2^-24 ~ 1e-6 at these pixel counts, plus one float32 rounding of the result;
          the accumulators here are float64.  Held to 2e-6 relative against the recorded value, and to 1e-12 relative against a float64
          mean of the bit-identical float32 per-pixel values (only the order of float64 additions differs).
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'metrics.npz')
REL_RECORDED = 2e-6
REL_FLOAT64 = 1e-12
FLOW_COUNT_COLS = (0, 2, 3, 4, 5, 6, 8, 10, 12, 14)
FLOW_SUM_COLS = (1, 7, 9, 11, 13, 15)
DISP_COUNT_COLS, DISP_SUM_COLS = (0, 2, 3, 4, 5, 6, 7), (1,)
DEPTH_COUNT_COLS, DEPTH_SUM_COLS = (0, 5, 6, 7), (1, 2, 3, 4)
SHARE_KEYS = ('1px', '3px', '5px', 'f1', 'd1', 'thres1', 'thres2', 'thres3', 'bad', 'a1', 'a2', 'a3')


def load_golden():
    return np.load(GOLDEN)


def check_share(value, recorded, what=''):
    recorded = np.asarray(recorded)
    tol = float(np.spacing(np.abs(recorded)))
    print(f'share {what}: {value!r} recorded {float(recorded)!r} ({recorded.dtype}) tol {tol:.3g}')
    assert abs(value - float(recorded)) <= tol, (what, value, float(recorded))


def check_sum(value, recorded, what='', rel=REL_RECORDED):
    recorded = float(np.asarray(recorded))
    err = abs(value - recorded) / abs(recorded)
    print(f'sum {what}: {value!r} against {recorded!r} rel {err:.3g} (bound {rel:g})')
    assert err <= rel, (what, value, recorded, err)


def check_result(key, value, recorded, what=''):
    (check_share if key in SHARE_KEYS else check_sum)(value, recorded, f'{what}{key}')


def check_rows(got, want, count_cols, sum_cols, what=''):
    """Count accumulators equal exactly, sum accumulators within 1e-12 relative (NaN and inf must match as such)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got[:, count_cols], want[:, count_cols]), (what, got[:, count_cols], want[:, count_cols])
    g, w = got[:, sum_cols], want[:, sum_cols]
    finite = np.isfinite(w)
    assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~finite & ~np.isnan(w)], w[~finite & ~np.isnan(w)]), (what, g, w)
    err = np.abs(g[finite] - w[finite]) / np.maximum(np.abs(w[finite]), 1e-300)
    print(f'rows {what}: largest relative difference of a sum {err.max() if err.size else 0.0:.3g}')
    assert (err <= REL_FLOAT64).all(), (what, err.max())


def flow_pixels(pred, gt, crop=(0, 0)):
    """Per-pixel float32 (epe, mag) of one sample, in NumPy: separately rounded products and sums, correctly rounded square roots."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    h, w = gt.shape[-2:]
    p = pred[:, crop[0]:crop[0] + h, crop[1]:crop[1] + w]
    du, dv = p[0] - gt[0], p[1] - gt[1]
    epe = np.sqrt(du * du + dv * dv)
    mag = np.sqrt(gt[0] * gt[0] + gt[1] * gt[1])
    assert epe.dtype == np.float32 and mag.dtype == np.float32
    return epe, mag


def seeded_flow_case(b, h, w, seed, sparse=False):
    """Ground truth with all three speed bins, motionless and out-of-frame pixels; an unpadded prediction; valid; noc_valid."""
    g = torch.Generator().manual_seed(seed)
    ramp = torch.linspace(0, 1, w).view(1, 1, 1, w)
    ang = torch.rand(b, 1, 1, 1, generator=g) * 6.283
    speed = 70.0 * ramp ** 2 * (0.8 + 0.4 * torch.rand(b, 1, h, 1, generator=g))
    gt = torch.cat([speed * torch.cos(ang), speed * torch.sin(ang)], 1) + 0.3 * torch.randn(b, 2, h, w, generator=g)
    gt[:, :, 5:12, 3:9] = 0.0
    gt[:, 0, 20:24, :6] = -9.0
    gt = gt.float().contiguous()
    pred = gt + torch.randn(b, 2, h, w, generator=g) * (0.2 + 6.0 * torch.rand(b, 1, h, w, generator=g))
    pred[:, :, 5:8, 3:9] = 0.0
    valid = (torch.rand(b, h, w, generator=g) < (0.3 if sparse else 0.97)).float()
    noc = (torch.rand(b, h, w, generator=g) > 0.25).float()
    return pred.float().contiguous(), gt, valid, noc
