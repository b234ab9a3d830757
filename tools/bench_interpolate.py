"""Cost of the frame-synthesis kernels against the same computation as torch ops on the same GPU.

    python tools/bench_interpolate.py [--out profiles/interpolate.txt] [--pairs 8]

Rows: 436 x 1024 and 1080 x 1920, 8 pairs, K = 1 and K = 3 in-between frames per pair, fp32 NCHW frames.

  warp      ``um_image_warp`` (zeros padding)                         | ``F.grid_sample`` on the normalised grid (the reference's flow_warp)
  splat     ``um_flow_splat``: the clear of the accumulators and one  | the same integer sums with ``index_put_(accumulate=True)`` on
            launch over both directions and all K times               |   int64, one call per plane, tap, time and direction
  synth     ``um_frame_synthesize`` on given accumulators             | float64 normalisation, ``where`` chains, four ``grid_sample`` calls
                                                                      |   per time (two frames with border padding, two masks), blend
  together  ``interp.interpolate_frames`` (splat + synth)             | splat + synth of the torch composition

The two legs of an operation alternate inside one process after a warm-up of both; a region is as many calls as last at least 0.25 s,
timed with device events; the figure is the median of the regions.  The torch composition is written plainly and is not tuned; it is
checked against the kernels before anything is timed: the integer sums exactly; the frames to one grey level on at most 5 % of the
values (``grid_sample`` weighs its taps in another order) and more than that on at most 0.1 % (an in-frame decision that falls the
other way in the last bit); the kernel itself is compared bit for bit with the host restatement on the first pair.  "atomic rate" is the bytes the splat launch adds -- 3 planes x 8 B per in-frame tap of non-zero
weight, counted from the inputs -- over the time of the whole ``um_flow_splat`` call, its clear included.
"""
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unimatch_amd import _abi, interp, video  # noqa: E402

ARGV = sys.argv[1:]
REGIONS = 5
REGION_SECONDS = 0.25
DEV = 'cuda'


def arg(name, default):
    return type(default)(ARGV[ARGV.index(name) + 1]) if name in ARGV else default


def timed(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e-3 / calls


def alternate(fns):
    calls = {}
    for k, fn in fns.items():
        timed(fn, 2)
        calls[k] = max(1, int(REGION_SECONDS / timed(fn, 2)) + 1)
    times = {k: [] for k in fns}
    for _ in range(REGIONS):
        for k, fn in fns.items():
            times[k].append(timed(fn, calls[k]))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


# ------------------------------------------------------------------ the torch composition
def grid_xy(h, w):
    ys, xs = torch.meshgrid(torch.arange(h, device=DEV, dtype=torch.float32), torch.arange(w, device=DEV, dtype=torch.float32), indexing='ij')
    return xs[None], ys[None]


def sample_torch(img, x, y, padding):
    h, w = img.shape[-2:]
    grid = torch.stack([2 * x / (w - 1) - 1, 2 * y / (h - 1) - 1], -1)
    return F.grid_sample(img, grid, mode='bilinear', padding_mode=padding, align_corners=True)


def warp_torch(img, flow):
    x, y = grid_xy(*flow.shape[-2:])
    return sample_torch(img, x + flow[:, 0], y + flow[:, 1], 'zeros')


def splat_torch(flow, times, count=False):
    """int64 ``[B, K, 3, H, W]`` by ``index_put_(accumulate=True)``; with ``count`` also the number of adds per plane."""
    b, _, h, w = flow.shape
    u, v = flow[:, 0], flow[:, 1]
    ok = (u.abs() <= 32768) & (v.abs() <= 32768)
    u, v = torch.where(ok, u, torch.zeros_like(u)), torch.where(ok, v, torch.zeros_like(v))
    uq, vq = torch.round(u * 256.0).long(), torch.round(v * 256.0).long()
    x, y = grid_xy(h, w)
    bi = torch.arange(b, device=DEV).view(b, 1, 1).expand(b, h, w)
    acc = torch.zeros(b, len(times), 3, h, w, dtype=torch.int64, device=DEV)
    adds = 0
    for kk, t in enumerate(times):
        t = float(t)
        X, Y = x + t * u, y + t * v
        fx0, fy0 = torch.floor(X), torch.floor(Y)
        ax, ay = X - fx0, Y - fy0
        x0, y0 = fx0.long(), fy0.long()
        for dy, dx, wt in ((0, 0, (1 - ax) * (1 - ay)), (0, 1, ax * (1 - ay)), (1, 0, (1 - ax) * ay), (1, 1, ax * ay)):
            wq = torch.round(wt * 65536.0).long()
            yy, xx = y0 + dy, x0 + dx
            hit = ok & (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w) & (wq > 0)
            wq = torch.where(hit, wq, torch.zeros_like(wq))
            yy, xx = yy.clamp(0, h - 1), xx.clamp(0, w - 1)
            for plane, val in enumerate((wq, wq * uq, wq * vq)):
                acc[:, kk, plane].index_put_((bi, yy, xx), val, accumulate=True)
            if count:
                adds += int(hit.sum())
    return (acc, adds) if count else acc


def synth_torch(img0, img1, acc_f, acc_b, times, occ_f, occ_b, thr=256):
    b, _, h, w = img0.shape
    x, y = grid_xy(h, w)
    frames = []
    for kk, t in enumerate(times):
        t = float(t)
        t1 = float(np.float32(1) - np.float32(t))
        est = []
        for acc in (acc_f, acc_b):
            sw = acc[:, kk, 0]
            valid = sw >= thr
            den = torch.where(valid, sw, torch.ones_like(sw)).double()
            est.append((valid, (acc[:, kk, 1].double() / den / 256.0).float(), (acc[:, kk, 2].double() / den / 256.0).float()))
        (va, au, av), (vb, bu, bv) = est
        zero = torch.zeros_like(au)
        mu = torch.where(va & vb, 0.5 * (au - bu), torch.where(va, au, torch.where(vb, -bu, zero)))
        mv = torch.where(va & vb, 0.5 * (av - bv), torch.where(va, av, torch.where(vb, -bv, zero)))
        x0, y0, x1, y1 = x - t * mu, y - t * mv, x + t1 * mu, y + t1 * mv
        v0 = ((x0 >= 0) & (x0 <= w - 1) & (y0 >= 0) & (y0 <= h - 1)).float()
        v1 = ((x1 >= 0) & (x1 <= w - 1) & (y1 >= 0) & (y1 <= h - 1)).float()
        c0, c1 = sample_torch(img0, x0, y0, 'border'), sample_torch(img1, x1, y1, 'border')
        o0, o1 = sample_torch(occ_f[:, None], x0, y0, 'zeros')[:, 0], sample_torch(occ_b[:, None], x1, y1, 'zeros')[:, 0]
        w0, w1 = t1 * v0 * (1 - o1), t * v1 * (1 - o0)
        plain = (w0 + w1) < 1e-6
        w0, w1 = torch.where(plain, torch.full_like(w0, t1), w0), torch.where(plain, torch.full_like(w1, t), w1)
        val = (w0[:, None] * c0 + w1[:, None] * c1) / (w0 + w1)[:, None]
        frames.append(torch.round(val).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1))
    return torch.stack(frames, 1)


# ------------------------------------------------------------------ the rows
def smooth(b, h, w, seed, amp):
    g = torch.Generator().manual_seed(seed)
    return (F.interpolate(torch.randn(b, 2, 6, 9, generator=g), (h, w), mode='bilinear', align_corners=True) * amp).to(DEV).contiguous()


def row(lines, pairs, h, w, k):
    lib = _abi.load()
    stream = torch.cuda.current_stream().cuda_stream
    times = interp._times32(interp.between_times(k))
    t1 = np.float32(1.0) - times
    fwd = smooth(pairs, h, w, 1, 6.0) + torch.tensor([3.0, -1.5], device=DEV).view(1, 2, 1, 1)
    bwd = (-fwd + smooth(pairs, h, w, 2, 0.4)).contiguous()
    g = torch.Generator().manual_seed(3)
    img0 = torch.randint(0, 256, (pairs, 3, h, w), generator=g).float().to(DEV)
    img1 = torch.randint(0, 256, (pairs, 3, h, w), generator=g).float().to(DEV)
    occ_f, occ_b = video.forward_backward_consistency_check(fwd, bwd)
    acc = torch.empty((2, pairs, k, 3, h, w), dtype=torch.int64, device=DEV)
    out = torch.empty((pairs, k, h, w, 3), dtype=torch.uint8, device=DEV)
    warped = torch.empty_like(img1)
    both, tptr = interp._host_times([times, t1])

    def k_warp():
        _abi.check(lib.um_image_warp(img1.data_ptr(), 0, fwd.data_ptr(), warped.data_ptr(), None, pairs, 3, h, w, 0, stream), 'warp')

    def k_splat():
        _abi.check(lib.um_flow_splat(fwd.data_ptr(), bwd.data_ptr(), None, None, tptr, pairs, k, h, w, 1.0 / 256, None, None, acc.data_ptr(),
                                     acc.numel() * 8, stream), 'splat')

    def k_synth():
        _abi.check(lib.um_frame_synthesize(img0.data_ptr(), img1.data_ptr(), 0, occ_f.data_ptr(), occ_b.data_ptr(), tptr, acc.data_ptr(),
                                           acc.numel() * 8, out.data_ptr(), None, pairs, k, h, w, 1.0 / 256, stream), 'synth')

    def k_together():
        return interp.interpolate_frames(img0, img1, fwd, bwd, list(times), occ_fwd=occ_f, occ_bwd=occ_b)

    def t_splat():
        return splat_torch(fwd, times), splat_torch(bwd, t1)

    # the composition computes what the kernels compute
    k_splat()
    (ref_f, adds_f), (ref_b, adds_b) = splat_torch(fwd, times, count=True), splat_torch(bwd, t1, count=True)
    assert torch.equal(acc[0], ref_f) and torch.equal(acc[1], ref_b), 'the torch splat disagrees with um_flow_splat'
    k_synth()
    ref = synth_torch(img0, img1, ref_f, ref_b, times, occ_f, occ_b)
    # the kernel is the host restatement bit for bit at this size too (first pair) ...
    host = interp.interpolate_frames(img0[:1].cpu(), img1[:1].cpu(), fwd[:1].cpu(), bwd[:1].cpu(), list(times), occ_fwd=occ_f[:1].cpu(),
                                     occ_bwd=occ_b[:1].cpu())
    assert torch.equal(out[:1].cpu(), host), 'um_frame_synthesize disagrees with the host restatement'
    # ... and the torch composition computes the same thing: one grey level apart at most, except where one of its discontinuous
    # decisions (is the sample position inside the frame) falls the other way in the last bit (its element-wise kernels contract
    # x - t * m into a fused multiply-add)
    off = (out.int() - ref.int()).abs()
    share, far = float((off > 0).float().mean()), float((off > 1).float().mean())
    print(f'{h} x {w} K = {k}: torch synthesis vs kernel: {share:.3%} of the values differ, {far:.3%} by more than one grey level', flush=True)
    assert share < 0.05 and far < 0.001, 'the torch synthesis disagrees with um_frame_synthesize'
    k_warp()
    # (white-noise frames: a last-bit difference of the normalised coordinate is 1e-4 px at this width, times 255 per pixel)
    assert float((warped - warp_torch(img1, fwd)).abs().max()) < 0.5, 'grid_sample disagrees with um_image_warp'
    del ref, off

    legs = {'warp': (k_warp, lambda: warp_torch(img1, fwd)), 'splat': (k_splat, t_splat),
            'synth': (k_synth, lambda: synth_torch(img0, img1, ref_f, ref_b, times, occ_f, occ_b)),
            'together': (k_together, lambda: synth_torch(img0, img1, splat_torch(fwd, times), splat_torch(bwd, t1), times, occ_f, occ_b))}
    lines.append(f'{h} x {w}, {pairs} pairs, K = {k}   (accumulators {acc.numel() * 8 / 1e6:.0f} MB)')
    slower = []
    for name, (kernel, torch_leg) in legs.items():
        t = alternate({'kernel': kernel, 'torch': torch_leg})
        km, tm = t['kernel'][0], t['torch'][0]
        lines.append(f'  {name:<9} kernel {km * 1e6:10.1f} us [{t["kernel"][1] * 1e6:.1f} .. {t["kernel"][2] * 1e6:.1f}]   torch {tm * 1e6:11.1f} us '
                     f'[{t["torch"][1] * 1e6:.1f} .. {t["torch"][2] * 1e6:.1f}]   torch / kernel {tm / km:7.2f} x'
                     + ('' if km < tm else '   THE KERNEL IS SLOWER'))
        if km >= tm:
            slower.append(name)
        if name == 'splat':
            added = (adds_f + adds_b) * 3 * 8
            lines.append(f'            {adds_f + adds_b} taps -> {added / 1e6:.0f} MB of 64-bit integer atomic adds: {added / km / 1e12:.3f} TB/s '
                         f'over the whole call (clear of {acc.numel() * 8 / 1e6:.0f} MB included)')
    lines.append('')
    print('\n'.join(lines[-7:]), flush=True)
    return slower


def main():
    pairs = arg('--pairs', 8)
    out_path = arg('--out', os.path.join(ROOT, 'profiles', 'interpolate.txt'))
    lines = ['tools/bench_interpolate.py: frame-synthesis kernels against a torch-op composition of the same computation',
             f'device: {torch.cuda.get_device_name(0)}; median of {REGIONS} regions of >= {REGION_SECONDS} s per leg, legs alternating', '']
    slower = []
    for h, w in ((436, 1024), (1080, 1920)):
        for k in (1, 3):
            slower += [f'{h}x{w} K={k} {name}' for name in row(lines, pairs, h, w, k)]
            torch.cuda.empty_cache()
    lines.append('every row: the kernels are faster than the torch composition' if not slower else
                 'NOT faster than the torch composition: ' + ', '.join(slower))
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(lines[-1])


if __name__ == '__main__':
    main()
