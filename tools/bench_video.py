"""Video throughput: the pairwise protocol callers run today against ``UniMatch.forward_sequence`` (each frame encoded once), and the
post-processing (occlusion masks + flow colouring) on the library's kernels against the reference-style path.

    python tools/bench_video.py [--out profiles/video_bench.json] [--pairs 32]
    python tools/bench_video.py --kernels-only        # (under rocprofv3 --kernel-trace --stats) the two post-processing kernels only

Rows (GMFlow scale 1, seeded moving-texture frames from ``synth.synth_frames``), each in exact and fast precision:
  B = 8 and B = 1 at 512 x 768, B = 1 at 720 x 1280.
(A) ``model(frames[i:i+B], frames[i+1:i+B+1])`` stepping B over P pairs; (B) ``forward_sequence(frames, pairs_per_launch=B)`` over the same
P pairs (P + 1 frames).  A and B alternate in one process; each is timed as a synchronised region (synchronize, wall clock, synchronize,
as bench.py times its regions); the median of 3 regions per leg is reported, in pairs/s.
"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unimatch_amd import UniMatch, video  # noqa: E402
from unimatch_amd.synth import CONFIGS, synth_frames, synth_state_dict  # noqa: E402

ARGV = sys.argv[1:]


def arg(name, default):
    return type(default)(ARGV[ARGV.index(name) + 1]) if name in ARGV else default


HBM_TBS = 6.3                 # achievable HBM rate (TB/s) the kernel rows are compared with


def region(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(fns, reps=3):
    """Median wall time of each callable over ``reps`` synchronised regions, the callables alternating."""
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(region(fn))
    return {k: statistics.median(v) for k, v in times.items()}


def model_for(precision):
    ck, fk = CONFIGS['gmflow_s1']
    model = UniMatch(**ck).eval()
    model.load_state_dict(synth_state_dict({k: v.shape for k, v in model.state_dict().items()}))
    return model.cuda().set_precision(precision), {k: v for k, v in fk.items() if k != 'task'}


def throughput_row(model, kw, b, h, w, pairs):
    pairs = max(b, pairs - pairs % b)
    frames = synth_frames(pairs + 1, h, w, seed=4).cuda()

    def pairwise():
        for i in range(0, pairs, b):
            model(frames[i:i + b], frames[i + 1:i + b + 1], **kw)

    def sequence():
        model.forward_sequence(frames, pairs_per_launch=b, **kw)

    pairwise()                                        # warm-up: caches, first-call-sequential parts
    sequence()
    pairwise()
    sequence()
    t = alternate({'pairwise': pairwise, 'sequence': sequence})
    return {'batch': b, 'height': h, 'width': w, 'pairs': pairs,
            'pairwise_pairs_per_s': pairs / t['pairwise'], 'sequence_pairs_per_s': pairs / t['sequence'],
            'speedup': t['pairwise'] / t['sequence'], 'pairwise_ms_per_pair': 1e3 * t['pairwise'] / pairs,
            'sequence_ms_per_pair': 1e3 * t['sequence'] / pairs}


def post_rows(model, kw, pairs):
    """B = 8, 512 x 768, bidirectional: the step with and without occlusion + colouring, and the post-processing alone, on the kernels
    and the reference's way (torch grid_sample check on the device, flow copied to the host, NumPy colouring per image)."""
    b, h, w = 8, 512, 768
    pairs = max(b, pairs - pairs % b)
    frames = synth_frames(pairs + 1, h, w, seed=5).cuda()

    def plain():
        model.forward_sequence(frames, pairs_per_launch=b, pred_bidir_flow=True, **kw)

    def post():
        model.forward_sequence(frames, pairs_per_launch=b, pred_bidir_flow=True, consistency_check=True, colorize=True, **kw)

    for fn in (plain, post, plain, post):
        fn()
    t = alternate({'plain': plain, 'post': post})
    out = model.forward_sequence(frames[:b + 1], pairs_per_launch=b, pred_bidir_flow=True, **kw)
    fwd, bwd = out['flow'], out['flow_bwd']

    def kernels():
        video.forward_backward_consistency_check(fwd, bwd)
        video.flow_to_image(fwd)
        video.flow_to_image(bwd)

    def reference_style():
        video._occlusion_host(fwd, bwd, 0.01, 0.5)[0].cpu()
        for f in (fwd, bwd):
            host = f.permute(0, 2, 3, 1).cpu().numpy()
            for img in host:
                video._flow_to_image_host(img)

    kernels()
    reference_style()
    tk = alternate({'kernels': kernels, 'reference_style': reference_style})
    return {'batch': b, 'height': h, 'width': w, 'pairs': pairs, 'bidirectional': True,
            'step_ms_per_pair_plain': 1e3 * t['plain'] / pairs, 'step_ms_per_pair_with_post': 1e3 * t['post'] / pairs,
            'post_overhead': t['post'] / t['plain'] - 1.0,
            'post_kernels_ms_per_8_pairs': 1e3 * tk['kernels'], 'post_reference_style_ms_per_8_pairs': 1e3 * tk['reference_style']}


def kernels_only(reps=50):
    """The two post-processing kernels at 8 x 512 x 768, ``reps`` times each (for rocprofv3 --kernel-trace --stats).  The flows are
    smooth fields (bilinear upsampling of a 1/32 noise grid, 8 px rms, plus 0.5 px noise) as predicted flows are: per-pixel noise
    would scatter the occlusion kernel's bilinear taps over 64 cache lines per wave instruction."""
    g = torch.Generator().manual_seed(1)
    coarse = torch.randn(8, 2, 16, 24, generator=g) * 8
    fwd = torch.nn.functional.interpolate(coarse, size=(512, 768), mode='bilinear', align_corners=True)
    fwd = fwd + 0.5 * torch.randn(fwd.shape, generator=g)
    bwd = (-fwd + torch.randn(8, 2, 512, 768, generator=g)).cuda()
    fwd = fwd.contiguous().cuda()
    for _ in range(reps):
        video.forward_backward_consistency_check(fwd, bwd)
        video.flow_to_image(fwd)
    torch.cuda.synchronize()
    px = 8 * 512 * 768
    # algorithmic bytes: occlusion reads both flows once and writes both masks (the bilinear taps re-read cached lines);
    # colouring: the partial-maximum pass reads the flow, the colour pass reads it again and writes 3 bytes per pixel
    print(json.dumps({'pixels': px, 'bytes': {'fwd_bwd_occ_kernel': px * (16 + 8), 'flow_rgb_max_kernel': px * 8,
                                              'flow_rgb_kernel': px * (8 + 3)}}))


def kernel_rows(stats_csv, bytes_of):
    """Per-kernel rows from a rocprofv3 kernel_stats.csv: mean us and algorithmic bytes / time against HBM_TBS."""
    import csv
    rows = {}
    with open(stats_csv) as f:
        for r in csv.DictReader(f):
            for k, nbytes in bytes_of.items():
                if r['Name'].startswith(k):
                    us = float(r['AverageNs']) / 1e3
                    rows[k] = {'calls': int(r['Calls']), 'mean_us': us, 'bytes': nbytes,
                               'tb_per_s': nbytes / (us * 1e-6) / 1e12, 'fraction_of_hbm': nbytes / (us * 1e-6) / 1e12 / HBM_TBS}
    return rows


def main():
    if '--kernels-only' in ARGV:
        kernels_only(arg('--reps', 50))
        return
    if '--kernel-stats' in ARGV:                      # --kernel-stats STATS_CSV BYTES_JSON_LINE_FILE OUT_JSON: merge into OUT_JSON
        i = ARGV.index('--kernel-stats')
        stats, bytes_file, out = ARGV[i + 1:i + 4]
        with open(bytes_file) as f:
            meta = json.loads([ln for ln in f if ln.startswith('{')][-1])
        rows = kernel_rows(stats, meta['bytes'])
        data = json.load(open(out)) if os.path.exists(out) else {}
        data['kernels_8x512x768_rocprofv3'] = {'achievable_hbm_tb_per_s': HBM_TBS, 'rows': rows}
        with open(out, 'w') as f:
            json.dump(data, f, indent=1)
        print(json.dumps(rows, indent=1))
        return
    out_path = arg('--out', os.path.join(ROOT, 'profiles', 'video_bench.json'))
    pairs = arg('--pairs', 32)
    rows = []
    shapes = [(8, 512, 768), (1, 512, 768), (1, 720, 1280)]
    data = {'device': torch.cuda.get_device_name(0), 'config': 'gmflow_s1', 'timing': 'median of 3 synchronised regions, A/B alternated',
            'rows': rows}
    for precision in ('exact', 'fast'):
        model, kw = model_for(precision)
        for b, h, w in shapes:
            n = pairs if b > 1 else max(4, pairs // 4)
            row = dict(throughput_row(model, kw, b, h, w, n), precision=precision)
            rows.append(row)
            print(json.dumps(row), flush=True)
        if precision == 'exact':
            data['post_processing'] = post_rows(model, kw, pairs)
            print(json.dumps(data['post_processing']), flush=True)
        del model
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    prev = json.load(open(out_path)) if os.path.exists(out_path) else {}
    prev.update(data)
    with open(out_path, 'w') as f:
        json.dump(prev, f, indent=1)


if __name__ == '__main__':
    main()
