"""Evaluation metrics of the reference's validation loops as accumulators that stay on the device.

  FlowMetrics     validate_sintel / validate_kitti (evaluate_flow.py:349-638): EPE, 1 / 3 / 5 px, F1, speed bins, matched / unmatched
  StereoMetrics   loss/stereo_metric.py under the masks of evaluate_stereo.py: EPE, D1, thres 1 / 2 / 3, bad pixels
  DepthMetrics    compute_errors (loss/depth_loss.py:6-24): abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3

``update(pred, gt, ...)`` takes the batch as the model returned it, still padded; ``padder`` (an :class:`unimatch_amd.io.InputPadder`)
supplies the crop, which the kernel applies while it reads: nothing is unpadded into a copy.  For CUDA tensors ``update`` enqueues one
HIP call (``um_flow_metrics`` / ``um_disp_metrics`` / ``um_depth_metrics``: one row of float64 accumulators per sample) and keeps the
rows on the device; it does not synchronise and copies nothing to the host.  ``compute()`` is the only point that reads back.

For host tensors ``update`` runs the host restatement below, written step by step in the dtypes the reference evaluates in (float32
per pixel, through the same torch / NumPy operations); it produces the same rows, with float64 sums of the float32 per-pixel values
where the reference pools them in float32.  The CPU tests pin it against results recorded from the reference (tests/golden/metrics.npz),
the GPU tests pin the kernels against it.

Because rows are per sample, results do not depend on how samples were batched.
"""
import numpy as np
import torch

FLOW_K, DISP_K, DEPTH_K = 16, 8, 8

_hip_ops = None


def _hip():
    global _hip_ops
    if _hip_ops is None:
        from .ops import HipOps            # raises when the HIP extension or the GPU is missing: there is no silent fallback
        _hip_ops = HipOps()
    return _hip_ops


def _crop(pred, gt, padder):
    """``(top, left)`` of the ground-truth frame inside the padded prediction."""
    (hp, wp), (h, w) = pred.shape[-2:], gt.shape[-2:]
    if padder is None:
        if (hp, wp) != (h, w):
            raise ValueError(f'prediction {hp}x{wp} and ground truth {h}x{w} differ in size: pass the InputPadder that padded the images')
        return 0, 0
    left, right, top, bottom = padder._pad
    if (h + top + bottom, w + left + right) != (hp, wp):
        raise ValueError(f'the padder pads {h}x{w} to {h + top + bottom}x{w + left + right}, the prediction is {hp}x{wp}')
    return top, left


def _sum64(values, mask):
    """float64 sum of the float32 ``values`` under ``mask`` (NaN if a selected value is NaN)."""
    return values[mask].double().sum().item()


def _sqrt32(x):
    """The correctly rounded float32 square root, which is what the kernels compute (``__fsqrt_rn``) and what NumPy computes.
    ``Tensor.sqrt`` on the CPU may go through a vector maths library that is one ulp off for a fraction of a percent of its inputs
    (observed with an MKL build: 0.6 %), which moves a pooled mean by ~1e-9 relative: far inside the float32 pooling error of the
    reference's own results, but not inside the 1e-12 that ties the kernels to this restatement."""
    return torch.from_numpy(np.sqrt(x.contiguous().numpy()))


# ------------------------------------------------------------------ host restatements: one row per sample, as the kernels write them
def flow_rows_host(pred, gt, valid=None, noc_valid=None, crop=(0, 0)):
    """Rows ``[B, 16]`` float64 of ``um_flow_metrics`` (layout in include/unimatch_hip.h) from host tensors."""
    b, _, h, w = gt.shape
    top, left = crop
    pred, gt = pred.float(), gt.float()
    rows = torch.zeros(b, FLOW_K, dtype=torch.float64)
    ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing='ij')
    for i in range(b):
        flow = pred[i, :, top:top + h, left:left + w]                               # padder.unpad(flow_pr[0])
        epe = _sqrt32(torch.sum((flow - gt[i]) ** 2, dim=0))                          # float32, evaluate_flow.py:425 / :553
        mag = _sqrt32(torch.sum(gt[i] ** 2, dim=0))
        m = (valid[i] >= 0.5) if valid is not None else torch.ones(h, w, dtype=torch.bool)
        out = (epe > 3.0) & ((epe / mag) > 0.05)
        cols = [m.sum().item(), _sum64(epe, m), (m & (epe > 1)).sum().item(), (m & (epe > 3)).sum().item(),
                (m & (epe > 5)).sum().item(), (m & out).sum().item()]
        for sel in ((mag < 10), (mag >= 10) & (mag <= 40), (mag > 40)):
            cols += [(m & sel).sum().item(), _sum64(epe, m & sel)]
        if noc_valid is not None:
            cx, cy = xs + gt[i, 0], ys + gt[i, 1]                                     # compute_out_of_boundary_mask
            inframe = (cx >= 0) & (cx <= w - 1) & (cy >= 0) & (cy <= h - 1) & (gt[i, 0].abs() <= w - 1) & (gt[i, 1].abs() <= h - 1)
            mt = (noc_valid[i] > 0.5) & inframe
            cols += [(m & mt).sum().item(), _sum64(epe, m & mt), (m & ~mt).sum().item(), _sum64(epe, m & ~mt)]
        else:
            cols += [0, 0, 0, 0]
        rows[i] = torch.tensor(cols, dtype=torch.float64)
    return rows


def disp_rows_host(pred, gt, max_disp=0.0, crop=(0, 0)):
    """Rows ``[B, 8]`` float64 of ``um_disp_metrics`` from host tensors."""
    b, h, w = gt.shape
    top, left = crop
    pred, gt = pred.float(), gt.float()
    rows = torch.zeros(b, DISP_K, dtype=torch.float64)
    for i in range(b):
        est, d = pred[i, top:top + h, left:left + w], gt[i]
        m = d > 0
        if max_disp > 0:
            m = m & (d < max_disp)
        e = torch.abs(d - est)
        d1 = (e > 3) & (e / d > 0.05)
        bad = (e > 10) & (e / torch.maximum(d, torch.ones_like(d)) > 0.1)
        rows[i] = torch.tensor([m.sum().item(), _sum64(e, m), (m & (e > 1)).sum().item(), (m & (e > 2)).sum().item(),
                                (m & (e > 3)).sum().item(), (m & d1).sum().item(), (m & bad).sum().item(), 0], dtype=torch.float64)
    return rows


def depth_rows_host(pred, gt, valid=None, lo=0.0, hi=float('inf'), crop=(0, 0)):
    """Rows ``[B, 8]`` float64 of ``um_depth_metrics`` from host tensors (NumPy float32 per pixel, as compute_errors)."""
    b, h, w = gt.shape
    top, left = crop
    rows = torch.zeros(b, DEPTH_K, dtype=torch.float64)
    for i in range(b):
        est = pred[i, top:top + h, left:left + w].float().numpy()
        d = gt[i].float().numpy()
        m = (d > np.float32(lo)) & (d < np.float32(hi))
        if valid is not None:
            m = m & (valid[i].float().numpy() > 0.5)
        g, p = d[m], est[m]
        with np.errstate(all='ignore'):
            thresh = np.maximum(g / p, p / g)                                        # float32; NaN propagates, comparisons are false
            sq = (g - p) ** 2
            dl = np.log(g.astype(np.float64)) - np.log(p.astype(np.float64))
            cols = [g.size, (np.abs(g - p) / g).astype(np.float64).sum(), (sq / g).astype(np.float64).sum(),
                    sq.astype(np.float64).sum(), (dl * dl).sum(),
                    # weak Python scalars under NumPy 2 (and exactly representable ones under NumPy 1): float32 comparisons
                    (thresh < 1.25).sum(), (thresh < 1.25 ** 2).sum(), (thresh < 1.25 ** 3).sum()]
        rows[i] = torch.tensor([float(c) for c in cols], dtype=torch.float64)
    return rows


# ------------------------------------------------------------------ accumulators
def _ratio(num, den):
    return float(num / den) if den > 0 else float('nan')


class _RowAccumulator:
    """Rows of per-sample accumulators, kept where they were produced until :meth:`rows` reads them back."""

    K = 0

    def __init__(self):
        self._rows = []

    def rows(self):
        """``[N, K]`` float64 on the host, one row per sample in the order fed: the ONE read-back (a device-side concatenation and
        a single copy)."""
        if not self._rows:
            return np.zeros((0, self.K))
        devices = {r.device for r in self._rows}
        if len(devices) == 1:
            return torch.cat(self._rows, 0).cpu().numpy()
        return torch.cat([r.cpu() for r in self._rows], 0).numpy()

    @staticmethod
    def _like(t, ref):
        if t is None:
            return None
        if not torch.is_tensor(t):
            t = torch.as_tensor(t)
        if t.device != ref.device:
            t = t.to(ref.device, non_blocking=True)
        return t


class FlowMetrics(_RowAccumulator):
    """End-point-error statistics of optical flow.

    ``update(flow_pr, flow_gt, valid=None, noc_valid=None, padder=None)``: ``flow_pr [B, 2, Hp, Wp]`` as the model returned it,
    ``flow_gt [B, 2, H, W]``, ``valid`` / ``noc_valid`` ``[B, H, W]`` (float or bool).  Pixels with ``valid >= 0.5`` count (all of
    them without ``valid``: validate_sintel ignores the mask, validate_kitti applies it).  ``noc_valid`` adds matched / unmatched."""

    K = FLOW_K

    def __init__(self):
        super().__init__()
        self._noc = None

    def update(self, flow_pr, flow_gt, valid=None, noc_valid=None, padder=None):
        if flow_pr.dim() != 4 or flow_pr.shape[1] != 2 or flow_gt.dim() != 4 or flow_gt.shape[:2] != flow_pr.shape[:2]:
            raise ValueError(f'expected flow_pr [B, 2, Hp, Wp] and flow_gt [B, 2, H, W], got {tuple(flow_pr.shape)} and {tuple(flow_gt.shape)}')
        if self._noc is not None and self._noc != (noc_valid is not None):
            raise ValueError('noc_valid was given for some updates and not for others')
        self._noc = noc_valid is not None
        crop = _crop(flow_pr, flow_gt, padder)
        flow_gt, valid, noc_valid = (self._like(t, flow_pr) for t in (flow_gt, valid, noc_valid))
        for m in (valid, noc_valid):
            if m is not None and tuple(m.shape) != (flow_gt.shape[0],) + tuple(flow_gt.shape[-2:]):
                raise ValueError(f'expected masks [B, H, W], got {tuple(m.shape)}')
        if flow_pr.is_cuda:
            with torch.cuda.device(flow_pr.device):
                rows = _hip().flow_metrics(flow_pr.float(), flow_gt.float(), valid, noc_valid, crop)
        else:
            rows = flow_rows_host(flow_pr, flow_gt, None if valid is None else valid.float(),
                                  None if noc_valid is None else noc_valid.float(), crop)
        self._rows.append(rows)
        return self

    def compute(self, average_over_pixels=True):
        """Dict of Python floats: ``epe``, ``1px``, ``3px``, ``5px``, ``f1`` (100 x the outlier share), ``s0_10``, ``s10_40``,
        ``s40+``, with ``noc_valid`` also ``matched`` / ``unmatched``, and ``skipped``: the number of samples without a valid pixel,
        which contribute nothing (the reference would produce NaN for such a sample in per-sample mode).

        ``average_over_pixels=True`` pools pixels over all samples.  ``False`` reproduces validate_kitti's per-sample means: ``epe``
        is the mean of each sample's mean, each speed bin averages over the samples that have pixels in it; the shares and ``f1``
        stay pixel-pooled, as in the reference.  A statistic without any pixel is NaN.  matched / unmatched pool the samples that
        have a matched pixel (validate_sintel appends to both lists only then)."""
        r = self.rows()
        n = r[:, 0]
        keep = r[n > 0]
        out = {'skipped': int((n == 0).sum())}
        total = keep[:, 0].sum()
        if average_over_pixels:
            out['epe'] = _ratio(keep[:, 1].sum(), total)
        else:
            out['epe'] = float(np.mean(keep[:, 1] / keep[:, 0])) if len(keep) else float('nan')
        for name, col in (('1px', 2), ('3px', 3), ('5px', 4)):
            out[name] = _ratio(keep[:, col].sum(), total)
        out['f1'] = 100 * _ratio(keep[:, 5].sum(), total)
        for name, col in (('s0_10', 6), ('s10_40', 8), ('s40+', 10)):
            has = keep[keep[:, col] > 0]
            if average_over_pixels:
                out[name] = _ratio(has[:, col + 1].sum(), has[:, col].sum())
            else:
                out[name] = float(np.mean(has[:, col + 1] / has[:, col])) if len(has) else float('nan')
        if self._noc:
            has = keep[keep[:, 12] > 0]
            out['matched'] = _ratio(has[:, 13].sum(), has[:, 12].sum())
            out['unmatched'] = _ratio(has[:, 15].sum(), has[:, 14].sum())
        return out


class _PerSampleMeans(_RowAccumulator):
    """Results that are means of per-sample values over the samples whose mask is non-empty (the reference's stereo and depth
    validations ``continue`` past a sample without a valid pixel)."""

    def per_sample(self):
        raise NotImplementedError

    def compute(self):
        per = self.per_sample()
        skipped = per.pop('skipped')
        out = {k: (float(np.mean(v)) if len(v) else float('nan')) for k, v in per.items()}
        out['skipped'] = skipped
        return out


class StereoMetrics(_PerSampleMeans):
    """``epe``, ``d1``, ``thres1`` / ``thres2`` / ``thres3`` and ``bad`` (bad_pixel_metric at its default thresholds) of disparities
    ``pred [B, Hp, Wp]`` against ``gt [B, H, W]`` over ``gt > 0`` (and ``gt < max_disp`` when ``max_disp > 0``, as validate_things)."""

    K = DISP_K

    def __init__(self, max_disp=0.0):
        super().__init__()
        self.max_disp = float(max_disp)

    def update(self, pred, gt, padder=None):
        if pred.dim() != 3 or gt.dim() != 3 or pred.shape[0] != gt.shape[0]:
            raise ValueError(f'expected pred [B, Hp, Wp] and gt [B, H, W], got {tuple(pred.shape)} and {tuple(gt.shape)}')
        crop = _crop(pred, gt, padder)
        gt = self._like(gt, pred)
        if pred.is_cuda:
            with torch.cuda.device(pred.device):
                rows = _hip().disp_metrics(pred.float(), gt.float(), self.max_disp, crop)
        else:
            rows = disp_rows_host(pred, gt, self.max_disp, crop)
        self._rows.append(rows)
        return self

    def per_sample(self):
        """Per-sample values (arrays over the samples with a non-empty mask) and ``skipped``."""
        r = self.rows()
        keep = r[r[:, 0] > 0]
        n = keep[:, 0]
        out = {name: keep[:, col] / n for name, col in (('epe', 1), ('thres1', 2), ('thres2', 3), ('thres3', 4), ('d1', 5), ('bad', 6))}
        out['skipped'] = int(len(r) - len(keep))
        return out


class DepthMetrics(_PerSampleMeans):
    """``abs_rel``, ``sq_rel``, ``rmse``, ``rmse_log``, ``a1``, ``a2``, ``a3`` of depths ``pred [B, Hp, Wp]`` against
    ``gt [B, H, W]`` over ``min_depth < gt < max_depth`` and ``valid > 0.5``."""

    K = DEPTH_K

    def __init__(self, min_depth=0.0, max_depth=float('inf')):
        super().__init__()
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)

    def update(self, pred, gt, valid=None, padder=None):
        if pred.dim() != 3 or gt.dim() != 3 or pred.shape[0] != gt.shape[0]:
            raise ValueError(f'expected pred [B, Hp, Wp] and gt [B, H, W], got {tuple(pred.shape)} and {tuple(gt.shape)}')
        crop = _crop(pred, gt, padder)
        gt, valid = self._like(gt, pred), self._like(valid, pred)
        if valid is not None and valid.shape != gt.shape:
            raise ValueError(f'expected valid [B, H, W], got {tuple(valid.shape)}')
        if pred.is_cuda:
            with torch.cuda.device(pred.device):
                rows = _hip().depth_metrics(pred.float(), gt.float(), valid, self.min_depth, self.max_depth, crop)
        else:
            rows = depth_rows_host(pred, gt, valid, self.min_depth, self.max_depth, crop)
        self._rows.append(rows)
        return self

    def per_sample(self):
        r = self.rows()
        keep = r[r[:, 0] > 0]
        n = keep[:, 0]
        out = {'abs_rel': keep[:, 1] / n, 'sq_rel': keep[:, 2] / n, 'rmse': np.sqrt(keep[:, 3] / n), 'rmse_log': np.sqrt(keep[:, 4] / n),
               'a1': keep[:, 5] / n, 'a2': keep[:, 6] / n, 'a3': keep[:, 7] / n}
        out['skipped'] = int(len(r) - len(keep))
        return out
