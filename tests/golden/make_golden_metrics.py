"""Mint ``metrics.npz`` from the REAL reference (runs only where the reference checkout exists):

    python tests/golden/make_golden_metrics.py

Records what the reference's evaluation code returns for seeded inputs; inputs and recorded results only.

  flow    the formulas live inside ``evaluate_flow.validate_sintel`` / ``validate_kitti``, so those functions themselves are driven, on
          the CPU: empty stand-ins for the modules they import but do not need here (cv2, imageio, torchvision.transforms),
          ``Tensor.cuda`` returning ``self``, the dataset classes replaced by a small in-memory dataset, and a stub model whose i-th call
          returns a recorded prediction that was padded with the reference's own InputPadder for that mode.  Recorded: validate_sintel
          with the speed bins and matched / unmatched, validate_kitti with the speed bins pixel-pooled and per sample.
  stereo  ``loss.stereo_metric`` (epe, d1, thres 1 / 2 / 3, bad_pixel) per sample, under gt > 0 and under validate_things' gt < max_disp.
  depth   ``loss.depth_loss.compute_errors`` per sample under the mask of evaluate_depth.

Four 37 x 53 samples per set (odd, so that both pad modes pad; the reference's ``np.mean(epe_list)`` needs equal sizes).  The flows
reach all three speed bins in every sample, contain pixels with zero ground-truth motion (``epe / mag`` is inf or NaN there),
ground-truth targets that leave the frame and displacements larger than the frame; KITTI's ``valid`` is sparse.  The NumPy version
is stored next to the results (its promotion rules decide how ``thresh < 1.25 ** 2`` compares).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get('UNIMATCH_REFERENCE', '/root/reference')
sys.path.insert(0, REFERENCE)

N, H, W = 4, 37, 53


def stand_ins():
    cv2 = types.ModuleType('cv2')
    cv2.setNumThreads = lambda n: None
    cv2.ocl = types.SimpleNamespace(setUseOpenCL=lambda flag: None)
    sys.modules.setdefault('cv2', cv2)
    sys.modules.setdefault('imageio', types.ModuleType('imageio'))
    try:
        import torchvision.transforms  # noqa: F401
    except Exception:
        tv = types.ModuleType('torchvision')
        tr = types.ModuleType('torchvision.transforms')
        tr.ColorJitter = object
        tv.transforms = tr
        sys.modules['torchvision'] = tv
        sys.modules['torchvision.transforms'] = tr
    torch.Tensor.cuda = lambda self, *a, **k: self


def flow_set(seed):
    """Ground truth [N, 2, H, W], prediction [N, 2, H, W], noc_valid [N, H, W] of one dataset."""
    g = torch.Generator().manual_seed(seed)
    ramp = torch.linspace(0, 1, W).view(1, 1, 1, W)
    ang = torch.rand(N, 1, 1, 1, generator=g) * 2 * np.pi
    speed = 70.0 * ramp ** 2 * (0.8 + 0.4 * torch.rand(N, 1, H, 1, generator=g))       # 0 .. ~80 px: every speed bin in every sample
    gt = torch.cat([speed * torch.cos(ang), speed * torch.sin(ang)], 1) + 0.3 * torch.randn(N, 2, H, W, generator=g)
    gt[:, :, 5:12, 3:9] = 0.0                                                          # no motion at all: mag == 0
    gt[:, 0, 20:24, :6] = -9.0                                                         # leaves the frame on the left
    gt[:, 1, -3:, 10:20] = 7.5                                                         # ... and at the bottom
    gt[:, 0, 0:3, 30:34] = 60.0                                                        # |u| > W - 1: too large even where it lands inside
    gt = gt.float().contiguous()
    err = torch.randn(N, 2, H, W, generator=g) * torch.tensor([0.3, 1.0, 2.5, 6.0]).view(N, 1, 1, 1)
    err = err * (0.5 + 2.0 * torch.rand(N, 1, H, W, generator=g))
    pred = gt + err
    pred[:, :, 5:8, 3:9] = 0.0                                                         # exact where nothing moves: 0 / 0
    pred[:, 0, 8:10, 3:9] = 4.5                                                        # epe > 3 where mag == 0: inf > 0.05
    noc = (torch.rand(N, H, W, generator=g) > 0.25).float()
    return gt, pred.float().contiguous(), noc


class Pairs:
    """In-memory stand-in of the reference's datasets: items as MpiSintel / KITTI return them."""

    def __init__(self, gt, valid, noc=None):
        self.gt, self.valid, self.noc = gt, valid, noc

    def __len__(self):
        return self.gt.shape[0]

    def __getitem__(self, i):
        img = torch.zeros(3, H, W)
        item = (img, img.clone(), self.gt[i], self.valid[i])
        return item + (self.noc[i],) if self.noc is not None else item


class Stub:
    """The i-th call returns the i-th recorded (padded) prediction."""

    def __init__(self, padded):
        self.padded, self.calls = padded, 0

    def eval(self):
        return self

    def __call__(self, image1, image2, **kw):
        assert kw['task'] == 'flow' and tuple(image1.shape[-2:]) == tuple(self.padded.shape[-2:])
        out = self.padded[self.calls:self.calls + 1]
        self.calls += 1
        return {'flow_preds': [out]}


def as_arrays(prefix, results):
    return {f'{prefix}/{k}': np.asarray(v) for k, v in results.items()}


def main():
    stand_ins()
    import evaluate_flow
    from utils.utils import InputPadder
    from loss import stereo_metric
    from loss.depth_loss import compute_errors

    out = {'numpy_version': np.array(np.__version__), 'torch_version': np.array(torch.__version__)}

    # ---- Sintel: clean and final passes, valid is all ones in the dataset and the function ignores it
    sets = {d: flow_set(s) for d, s in (('clean', 101), ('final', 102))}
    pad = InputPadder((1, 3, H, W), padding_factor=8)
    padded = {d: pad.pad(v[1])[0] for d, v in sets.items()}
    evaluate_flow.MpiSintel = lambda split, dstype, load_occlusion: Pairs(sets[dstype][0], torch.ones(N, H, W), sets[dstype][2])
    res = evaluate_flow.validate_sintel(Stub(torch.cat([padded['clean'], padded['final']], 0)), with_speed_metric=True,
                                        evaluate_matched_unmatched=True)
    out.update(as_arrays('sintel', res))
    for d, (gt, _, noc) in sets.items():
        out[f'sintel_{d}_gt'], out[f'sintel_{d}_noc'], out[f'sintel_{d}_pred'] = gt.numpy(), noc.numpy(), padded[d].numpy()

    # ---- KITTI: sparse valid, all of the padding at the bottom
    gt, pred, _ = flow_set(103)
    valid = (torch.rand(N, H, W, generator=torch.Generator().manual_seed(104)) < 0.3).float()
    valid[:, 5:12, 3:9] = 1.0                                                          # the motionless patch is evaluated
    pad = InputPadder((1, 3, H, W), mode='kitti', padding_factor=8)
    padded_k = pad.pad(pred)[0]
    evaluate_flow.KITTI = lambda split: Pairs(gt, valid)
    out.update(as_arrays('kitti_pixels', evaluate_flow.validate_kitti(Stub(padded_k), with_speed_metric=True, average_over_pixels=True)))
    res = evaluate_flow.validate_kitti(Stub(padded_k), with_speed_metric=True, average_over_pixels=False)
    out.update(as_arrays('kitti_samples', {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in res.items()}))
    out['kitti_gt'], out['kitti_valid'], out['kitti_pred'] = gt.numpy(), valid.numpy(), padded_k.numpy()

    # ---- stereo: per-sample values of loss/stereo_metric.py under the masks of evaluate_stereo.py
    g = torch.Generator().manual_seed(105)
    disp = (torch.rand(N, H, W, generator=g) * 120.0).float()
    disp[:, :4] = 0.0                                                                  # invalid rows
    disp[:, 4:6] *= 0.005                                                              # disparities below 1: max(gt, 1) matters
    est = disp + torch.randn(N, H, W, generator=g) * torch.tensor([0.4, 1.5, 4.0, 14.0]).view(N, 1, 1)
    out['disp_gt'], out['disp_pred'] = disp.numpy(), est.float().numpy()
    out['disp_max_disp'] = np.array(80.0)
    for tag, masks in (('all', disp > 0), ('things', (disp > 0) & (disp < 80.0))):
        rec = {k: [] for k in ('epe', 'd1', 'thres1', 'thres2', 'thres3', 'bad')}
        for i in range(N):
            e, d, m = est[i].float(), disp[i], masks[i]
            rec['epe'].append(stereo_metric.epe_metric(e, d, m).numpy())
            rec['d1'].append(stereo_metric.d1_metric(e, d, m).numpy())
            for t in (1, 2, 3):
                rec[f'thres{t}'].append(stereo_metric.thres_metric(e, d, m, float(t)).numpy())
            rec['bad'].append(stereo_metric.bad_pixel_metric(e, d, m).numpy())
        out.update({f'disp_{tag}/{k}': np.stack(v) for k, v in rec.items()})

    # ---- depth: compute_errors(gt[mask], pred[mask]) per sample, mask = (gt > min) & (gt < max) & valid as evaluate_depth forms it
    g = torch.Generator().manual_seed(106)
    depth = (0.2 + 11.0 * torch.rand(N, H, W, generator=g)).float()
    dpred = (depth * torch.exp(torch.randn(N, H, W, generator=g) * torch.tensor([0.05, 0.15, 0.3, 0.6]).view(N, 1, 1))).float()
    dvalid = (torch.rand(N, H, W, generator=g) > 0.2).float()
    lo, hi = 0.5, 10.0
    out['depth_gt'], out['depth_pred'], out['depth_valid'] = depth.numpy(), dpred.numpy(), dvalid.numpy()
    out['depth_range'] = np.array([lo, hi])
    rec = []
    for i in range(N):
        d, p = depth[i].numpy(), dpred[i].numpy()
        m = (d > lo) & (d < hi) & (dvalid[i].numpy() > 0.5)
        rec.append([np.asarray(v) for v in compute_errors(d[m], p[m])])
    for j, name in enumerate(('abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'a1', 'a2', 'a3')):
        out[f'depth/{name}'] = np.stack([r[j] for r in rec])

    np.savez_compressed(os.path.join(HERE, 'metrics.npz'), **out)
    print({k: (v.shape, v.dtype) for k, v in out.items()})


if __name__ == '__main__':
    main()
