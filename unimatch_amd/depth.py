"""A posed-scene driver shaped like the reference's ``inference_depth`` (evaluate_depth.py:296-419).

``python -m unimatch_amd.depth --scene DIR --out DIR [...]`` reads a ScanNet-layout scene -- ``color/*.jpg|png`` (sorted),
``pose/*.txt`` (one 4 x 4 camera-to-world matrix per frame, sorted) and ``intrinsic/*.txt`` (a 4 x 4 file whose upper-left 3 x 3 is
used) -- predicts the depth of every frame i from the pair (i, i + 1) with :meth:`UniMatch.predict` and writes ``<stem>.png``: the
reference's ``viz_depth_tensor(1 / depth)`` colouring (:mod:`unimatch_amd.visualize`); with ``--pred-bidir-depth`` also
``<stem>_bwd.png``, the depth of frame i + 1.  The relative pose is ``inv(pose_tgt) @ pose_ref`` in float32 on the host; the model
searches the inverse depths ``1 / max_depth .. 1 / min_depth``.  Frames are uploaded as uint8 and normalised on the device; like the
reference's runner this one RESIZES (to the next multiple of ``padding_factor`` or to ``inference_size``) and does NOT rescale the
intrinsics; ``--scale-intrinsics`` opts into :meth:`InferenceGeometry.scaled_intrinsics`.  Reading frames needs PIL.

``--pairs-per-launch N`` runs the scene through :meth:`UniMatch.forward_sequence` (``task='depth'``) instead: every frame is read,
uploaded, prepared and encoded once, the absolute poses are uploaded once and the relative poses are formed on the device, N pairs go
through the match step per launch, and the coloured images come back once per piece of N pairs.  The files written are those of the
default mode; all frames must have one size.  ``--fuse-neighbours`` (with ``--pairs-per-launch``, not with ``--pred-bidir-depth``)
lets the previous frame vote in every frame's plane sweep as a second source view: the Transformer has already produced its tokens, so
it costs the sweep alone (``forward_sequence(fuse_neighbours=True)``; an unlearned fusion, the weights are trained on two views).

Values and geometry (both modes write the same files):

  ``--save-depth``          ``<stem>_depth.png``: the depth in millimetres as a 16-bit PNG, the format the reference's ScanNet loader
                            divides by 1000 (rounded, 0 where the depth is not finite; 65535 mm at most)
  ``--consistency-check``   ``<stem>_occ.png``: 255 where fewer than ``--min-views`` of the frame's neighbours (the previous and the next
                            frame) agree with its depth to ``--px-thr`` pixels and ``--rel-thr`` relative depth, 0 where the pixel is kept
  ``--save-ply FILE``       the fused, consistency-filtered, coloured world point cloud of the whole scene (binary PLY), every
                            ``--ply-stride``-th pixel of every row and column (:func:`unimatch_amd.geometry.fuse_depth_sequence`)
  ``--save-confidence``     ``<stem>_conf.png``: the plane sweep's ``max_prob`` (``UniMatch.forward_with_depth_confidence``, statistics
                            of the distribution over the depth candidates, window ``--peak-radius``), coloured per frame
  ``--min-confidence P``    with ``--save-ply``: a pixel also needs ``peak_mass >= P`` (the probability within ``--peak-radius``
                            candidates of the best one) -- a filter that needs no neighbouring frame.  With
                            ``--pred-bidir-depth`` the last frame's depth is the last pair's backward prediction: the pairwise mode
                            filters it on that prediction's own ``peak_mass``, ``--pairs-per-launch`` keeps the forward maps only
                            and leaves that one frame to the consistency check alone, so the two modes' clouds can differ in it
  ``--save-tsdf-ply FILE``  the TSDF surface of the whole scene (binary PLY): the same depths and colours fused in one voxel grid of
                            ``--voxel-size`` metres (:func:`unimatch_amd.fusion.fuse_depth_sequence_tsdf`), truncation
                            ``--tsdf-trunc`` (default: 4 voxels), the surface taken between voxels of weight ``>= --tsdf-min-weight``.
                            The integration weight is the ``keep`` mask of the point cloud -- consistency, plus ``--min-confidence``
                            when given -- so the surface is made of exactly the pixels ``--save-ply`` keeps, averaged across frames
                            instead of concatenated; it needs no ``--save-ply``
  ``--save-tsdf-mesh FILE`` the triangle mesh of that TSDF volume (binary PLY with a face element, :func:`unimatch_amd.io.write_ply_mesh`):
                            marching tetrahedra over the same volume, with the same ``--voxel-size``, ``--tsdf-trunc``,
                            ``--tsdf-min-weight`` and ``--min-confidence``; with ``--save-tsdf-ply`` as well, one volume serves both

Frame i has a depth map through the pair (i, i + 1); the last frame has one only with ``--pred-bidir-depth``, through the last pair's
backward prediction, and gets its ``_depth.png`` / ``_occ.png`` then.  The geometry always uses the depth restored to the frames' own
size with the scene's own intrinsics, whatever ``--scale-intrinsics`` gave the model.  For ``--consistency-check``, ``--save-ply`` and
``--save-tsdf-ply`` the runner keeps the restored depth maps and the uint8 frames of the whole scene resident on the device -- 4 + 3 bytes per pixel and frame
-- and fuses after the last piece (all frames of one size).
"""
import argparse
import glob
import os

import numpy as np
import torch

from .stereo import load_model, nearest_size
from .video import read_frame_u8
from .visualize import inverse_depth_to_image


def read_scene(scene_dir):
    """``(image paths, poses [N, 4, 4] float32, intrinsics [3, 3] float32)`` of a ScanNet-layout scene."""
    imgs = sorted(glob.glob(os.path.join(scene_dir, 'color', '*.jpg')) + glob.glob(os.path.join(scene_dir, 'color', '*.png')))
    poses = sorted(glob.glob(os.path.join(scene_dir, 'pose', '*.txt')))
    intr = sorted(glob.glob(os.path.join(scene_dir, 'intrinsic', '*.txt')))
    if not intr:
        raise FileNotFoundError(f'no intrinsic/*.txt under {scene_dir}')
    if len(imgs) != len(poses):
        raise ValueError(f'{len(imgs)} images and {len(poses)} poses under {scene_dir}')
    k = np.loadtxt(intr[0]).astype(np.float32).reshape(4, 4)[:3, :3]
    p = np.stack([np.loadtxt(f).astype(np.float32).reshape(4, 4) for f in poses], 0) if poses else np.zeros((0, 4, 4), np.float32)
    return imgs, p, k


def relative_pose(pose_ref, pose_tgt):
    """``inv(pose_tgt) @ pose_ref`` in float32 (evaluate_depth.py:347-350)."""
    return (np.linalg.inv(pose_tgt.astype(np.float32)) @ pose_ref.astype(np.float32)).astype(np.float32)


class _SceneCollector:
    """What ``--save-depth``, ``--consistency-check``, ``--save-ply`` and ``--save-tsdf-ply`` need of a scene: writes each restored depth map as it
    arrives and, for the latter two, keeps it and its uint8 frame on the device until :meth:`finish` fuses the scene."""

    def __init__(self, out_dir, imgs, poses, k, save_depth, consistency_check, save_ply, ply_stride, min_views, px_thr, rel_thr,
                 min_confidence=None, save_tsdf_ply=None, voxel_size=0.04, tsdf_trunc=None, tsdf_min_weight=1., save_tsdf_mesh=None):
        self.min_confidence, self.conf = min_confidence, []
        self.save_tsdf_mesh = save_tsdf_mesh
        self.save_tsdf_ply, self.voxel_size, self.tsdf_trunc, self.tsdf_min_weight = save_tsdf_ply, voxel_size, tsdf_trunc, tsdf_min_weight
        self.out_dir, self.imgs, self.poses, self.k = out_dir, imgs, poses, k
        self.save_depth, self.consistency_check, self.save_ply = save_depth, consistency_check, save_ply
        self.ply_stride, self.min_views, self.px_thr, self.rel_thr = ply_stride, min_views, px_thr, rel_thr
        self.fuse = bool(consistency_check or save_ply or save_tsdf_ply or save_tsdf_mesh)
        self.depths, self.frames = [], []

    def stem(self, i):
        return os.path.join(self.out_dir, os.path.splitext(os.path.basename(self.imgs[i]))[0])

    def add(self, i, depth, frame_u8, peak_mass=None):
        """Frame ``i`` (they arrive in order): its restored depth ``[H, W]`` fp32 and its frame ``[H, W, 3]`` uint8, on one device;
        ``peak_mass [H, W]`` at the frame's size when the cloud is filtered on it."""
        from .io import write_png16
        if self.save_depth:
            mm = torch.nan_to_num(depth * 1000., nan=0., posinf=0., neginf=0.).round().clamp(0., 65535.)
            write_png16(self.stem(i) + '_depth.png', mm.to(torch.int32).cpu().numpy().astype(np.uint16))
        if self.fuse:
            assert i == len(self.depths)
            if self.depths and depth.shape != self.depths[0].shape:
                raise ValueError(f'{self.imgs[i]} is {tuple(depth.shape)}, the scene began with {tuple(self.depths[0].shape)}: '
                                 '--consistency-check / --save-ply / --save-tsdf-ply need frames of one size')
            self.depths.append(depth)
            self.frames.append(frame_u8)
            if self.min_confidence is not None:
                self.conf.append(peak_mass)

    def finish(self):
        from .geometry import fuse_depth_sequence
        from .io import write_ply, write_png8
        if not self.fuse:
            return
        n = len(self.depths)
        if n < 2:
            raise ValueError(f'--consistency-check / --save-ply / --save-tsdf-ply need at least two frames with a depth map, the scene gave {n}')
        depths, colors = torch.stack(self.depths, 0), torch.stack(self.frames, 0)
        dev = depths.device
        out = fuse_depth_sequence(depths, torch.from_numpy(self.k)[None].to(dev), torch.from_numpy(self.poses[:n]).to(dev), colors,
                                  px_thr=self.px_thr, rel_thr=self.rel_thr, min_views=self.min_views, stride=self.ply_stride,
                                  **({} if self.min_confidence is None else
                                     {'confidence': torch.stack(self.conf, 0), 'min_confidence': self.min_confidence}))
        if self.consistency_check:
            occ = ((1. - out['keep']) * 255.).to(torch.uint8).cpu().numpy()
            for i in range(n):
                write_png8(self.stem(i) + '_occ.png', occ[i])
        if self.save_ply:
            write_ply(self.save_ply, out['xyz'].cpu().numpy(), out['rgb'].cpu().numpy())
        if self.save_tsdf_ply or self.save_tsdf_mesh:
            from .fusion import fuse_depth_sequence_tsdf
            from .io import write_ply_mesh
            if not bool(out['keep'].any()):                    # nothing is kept: an empty surface, as --save-ply writes an empty cloud
                if self.save_tsdf_ply:
                    write_ply(self.save_tsdf_ply, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
                if self.save_tsdf_mesh:
                    write_ply_mesh(self.save_tsdf_mesh, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32))
                return
            surf = fuse_depth_sequence_tsdf(depths, torch.from_numpy(self.k)[None].to(dev), torch.from_numpy(self.poses[:n]).to(dev), colors,
                                            weight=out['keep'], voxel_size=self.voxel_size, trunc=self.tsdf_trunc,
                                            min_weight=self.tsdf_min_weight, mesh=bool(self.save_tsdf_mesh))
            if self.save_tsdf_mesh:
                write_ply_mesh(self.save_tsdf_mesh, surf['xyz'].cpu().numpy(), surf['rgb'].cpu().numpy(), surf['faces'].cpu().numpy())
            if self.save_tsdf_ply:                             # the points of the same volume
                xyz, rgb = surf['volume'].extract_points(self.tsdf_min_weight) if self.save_tsdf_mesh else (surf['xyz'], surf['rgb'])
                write_ply(self.save_tsdf_ply, xyz.cpu().numpy(), rgb.cpu().numpy())


def run_depth(model, scene_dir, out_dir, fwd_kw, padding_factor=16, inference_size=None, min_depth=0.5, max_depth=10.,
              num_depth_candidates=64, depth_from_argmax=False, pred_bidir_depth=False, scale_intrinsics=False, device='cuda',
              pairs_per_launch=None, save_depth=False, consistency_check=False, save_ply=None, ply_stride=1, min_views=1, px_thr=1.0,
              rel_thr=0.01, save_confidence=False, min_confidence=None, peak_radius=1, fuse_neighbours=False, save_tsdf_ply=None,
              voxel_size=0.04, tsdf_trunc=None, tsdf_min_weight=1., save_tsdf_mesh=None):
    """``inference_depth`` over the scene: returns the number of frames written (one less than the scene has).
    ``pairs_per_launch=N``: sequence mode (the module docstring), in pieces of N pairs; ``None``: one ``predict`` per pair.
    ``save_depth``, ``consistency_check``, ``save_ply`` (a file name): the value and geometry outputs of the module docstring.
    ``save_tsdf_ply`` (a file name), ``voxel_size``, ``tsdf_trunc``, ``tsdf_min_weight``: the TSDF surface of the scene.
    ``save_tsdf_mesh`` (a file name): the triangle mesh of the same volume, with the same parameters.
    ``save_confidence``, ``min_confidence`` (with ``save_ply`` or ``save_tsdf_ply``), ``peak_radius``: the plane sweep's confidence, taken in the forward's
    own matching launch (``forward_with_depth_confidence`` / ``forward_sequence(return_confidence=True)``).
    ``fuse_neighbours`` (sequence mode only, not with ``pred_bidir_depth``): the previous frame votes in every frame's plane sweep
    (``forward_sequence(fuse_neighbours=True)``: an unlearned two-source fusion for the price of the sweep; the files are the same)."""
    from .confidence import confidence_to_image, confidence_to_image_size
    from .io import write_png8
    from .prepost import InferenceGeometry
    if min_confidence is not None and not (save_ply or save_tsdf_ply or save_tsdf_mesh):
        raise ValueError('min_confidence filters the point cloud: it needs save_ply, save_tsdf_ply or save_tsdf_mesh')
    if fuse_neighbours and pairs_per_launch is None:
        raise ValueError('fuse_neighbours is an option of the sequence mode: it needs pairs_per_launch')
    if fuse_neighbours and pred_bidir_depth:
        raise ValueError('fuse_neighbours replaces the backward prediction: it cannot be combined with pred_bidir_depth')
    want_conf = bool(save_confidence) or min_confidence is not None
    imgs, poses, k = read_scene(scene_dir)
    os.makedirs(out_dir, exist_ok=True)
    collect = None
    if save_depth or consistency_check or save_ply or save_tsdf_ply or save_tsdf_mesh:
        collect = _SceneCollector(out_dir, imgs, poses, k, save_depth, consistency_check, save_ply, int(ply_stride), int(min_views),
                                  float(px_thr), float(rel_thr), None if min_confidence is None else float(min_confidence),
                                  save_tsdf_ply, float(voxel_size), None if tsdf_trunc is None else float(tsdf_trunc),
                                  float(tsdf_min_weight), save_tsdf_mesh)
    skip = ('task', 'min_depth', 'max_depth', 'num_depth_candidates', 'depth_from_argmax', 'pred_bidir_depth', 'intrinsics', 'pose',
            'poses')
    fwd_kw = {key: v for key, v in fwd_kw.items() if key not in skip}
    if pairs_per_launch is not None:
        return _run_depth_sequence(model, imgs, poses, k, out_dir, fwd_kw, padding_factor, inference_size, min_depth, max_depth,
                                   num_depth_candidates, depth_from_argmax, pred_bidir_depth, scale_intrinsics, device,
                                   int(pairs_per_launch), collect, bool(save_confidence), want_conf, int(peak_radius),
                                   bool(fuse_neighbours))
    for i in range(len(imgs) - 1):
        ref, tgt = read_frame_u8(imgs[i])[None].to(device), read_frame_u8(imgs[i + 1])[None].to(device)
        size = tuple(inference_size) if inference_size else nearest_size(ref.shape[1:3], padding_factor)
        intrinsics = torch.from_numpy(k)[None].to(device)
        if scale_intrinsics:
            intrinsics = InferenceGeometry.resized(ref.shape[1:3], size).scaled_intrinsics(intrinsics)
        pose = torch.from_numpy(relative_pose(poses[i], poses[i + 1]))[None].to(device)
        depth_kw = dict(task='depth', intrinsics=intrinsics, pose=pose, min_depth=1. / max_depth, max_depth=1. / min_depth,
                        num_depth_candidates=num_depth_candidates, depth_from_argmax=depth_from_argmax, pred_bidir_depth=pred_bidir_depth,
                        **fwd_kw)
        peak = None
        with torch.no_grad():
            if want_conf:                      # predict()'s steps around the forward that also returns the statistics
                geom = InferenceGeometry.resized(ref.shape[1:3], size)
                a0, a1 = geom.prepare(ref, tgt, normalize=True)
                out = model.forward_with_depth_confidence(a0, a1, peak_radius=int(peak_radius), **depth_kw)
                depth = geom.restore(out['flow_preds'][-1], 'depth')
                conf = out['depth_confidence']
                if min_confidence is not None:
                    peak = confidence_to_image_size(conf['peak_mass'], conf['scale'], geom)
            else:
                depth = model.predict(ref, tgt, inference_size=size, **depth_kw)['flow_preds'][-1]
        rgb = inverse_depth_to_image(depth).cpu().numpy()                                    # [1 or 2, H, W, 3]
        stem = os.path.join(out_dir, os.path.splitext(os.path.basename(imgs[i]))[0])
        write_png8(stem + '.png', rgb[0])
        if pred_bidir_depth:
            write_png8(stem + '_bwd.png', rgb[1])
        if save_confidence:
            write_png8(stem + '_conf.png', confidence_to_image(conf['max_prob'][:1], tuple(ref.shape[1:3])).cpu().numpy()[0])
        if collect is not None:
            collect.add(i, depth[0], ref[0], None if peak is None else peak[0])
            if pred_bidir_depth and i == len(imgs) - 2:
                collect.add(i + 1, depth[1], tgt[0], None if peak is None else peak[1])
    if collect is not None:
        collect.finish()
    return max(0, len(imgs) - 1)


def _run_depth_sequence(model, imgs, poses, k, out_dir, fwd_kw, padding_factor, inference_size, min_depth, max_depth,
                        num_depth_candidates, depth_from_argmax, pred_bidir_depth, scale_intrinsics, device, step, collect=None,
                        save_confidence=False, want_conf=False, peak_radius=1, fuse_neighbours=False):
    """The scene through ``forward_sequence(task='depth')`` in pieces of ``step`` pairs (``step + 1`` frames first, then ``step`` frames
    joined by the carry), so that at most ``step + 1`` frames and their predictions are resident."""
    from .confidence import confidence_to_image, confidence_to_image_size
    from .io import write_png8
    from .prepost import InferenceGeometry
    if step < 1:
        raise ValueError('pairs_per_launch must be >= 1')
    if len(imgs) < 2:
        return 0
    geom = intrinsics = carry = shape = pending = None
    fuse_kw = {'fuse_neighbours': True} if fuse_neighbours else {}                           # the carry then joins the pieces' sweeps too
    pose_dev = torch.from_numpy(poses).to(device)                                            # absolute, uploaded once
    lo = 0
    while lo < len(imgs):
        hi = min(len(imgs), lo + step + (1 if carry is None else 0))
        host = [read_frame_u8(f) for f in imgs[lo:hi]]
        for f, frame in zip(imgs[lo:hi], host):
            shape = shape or tuple(frame.shape)
            if tuple(frame.shape) != shape:
                raise ValueError(f'{f} is {tuple(frame.shape[:2])}, the scene began with {shape[:2]}: --pairs-per-launch needs frames '
                                 'of one size')
        if geom is None:
            size = tuple(inference_size) if inference_size else nearest_size(shape[:2], padding_factor)
            geom = InferenceGeometry.resized(shape[:2], size)
            intrinsics = torch.from_numpy(k)[None].to(device)
            if scale_intrinsics:
                intrinsics = geom.scaled_intrinsics(intrinsics)
        frames_u8 = torch.stack(host, 0).to(device)
        frames, = geom.prepare(frames_u8, normalize=True)                                    # uint8 up, normalised on the device
        with torch.no_grad():
            out = model.forward_sequence(frames, task='depth', intrinsics=intrinsics, poses=pose_dev[lo:hi], carry=carry,
                                         pairs_per_launch=step, min_depth=1. / max_depth, max_depth=1. / min_depth,
                                         num_depth_candidates=num_depth_candidates, depth_from_argmax=depth_from_argmax,
                                         pred_bidir_depth=pred_bidir_depth, return_confidence=want_conf, peak_radius=peak_radius,
                                         **fuse_kw, **fwd_kw)
        carry = out['carry']
        first = lo - (0 if lo == 0 else 1)                                                   # the frame of the piece's first pair
        depth = [out['depth']] + ([out['depth_bwd']] if pred_bidir_depth else [])
        n = depth[0].shape[0]
        restored = geom.restore(torch.cat(depth, 0), 'depth')
        rgb = inverse_depth_to_image(restored).cpu().numpy()                                 # one copy back per piece
        for j in range(n):
            stem = os.path.join(out_dir, os.path.splitext(os.path.basename(imgs[first + j]))[0])
            write_png8(stem + '.png', rgb[j])
            if pred_bidir_depth:
                write_png8(stem + '_bwd.png', rgb[n + j])
        peak = None
        if want_conf:                                                                        # forward direction: the piece's n frames
            conf = out['depth_confidence']
            if save_confidence:
                crgb = confidence_to_image(conf['max_prob'], shape[:2]).cpu().numpy()
                for j in range(n):
                    write_png8(os.path.join(out_dir, os.path.splitext(os.path.basename(imgs[first + j]))[0]) + '_conf.png', crgb[j])
            if collect is not None and collect.min_confidence is not None:
                peak = confidence_to_image_size(conf['peak_mass'], conf['scale'], geom)
        if collect is not None:
            # the frames of the piece's pairs: the carried frame starts the first pair of every piece but the first
            pending = frames_u8 if first == lo else torch.cat([pending, frames_u8], 0)
            for j in range(n):
                collect.add(first + j, restored[j], pending[j], None if peak is None else peak[j])
            if pred_bidir_depth and hi == len(imgs):
                # the sequence keeps the forward maps only: the last frame, seen backward, passes the confidence filter unfiltered
                collect.add(first + n, restored[2 * n - 1], pending[n], None if peak is None else torch.ones_like(peak[0]))
            pending = pending[n:n + 1]                                                       # the last frame starts the next piece's first pair
        lo = hi
    if collect is not None:
        collect.finish()
    return len(imgs) - 1


def main(argv=None):
    from .synth import CONFIGS
    ap = argparse.ArgumentParser(description='depth of a posed ScanNet-layout scene (UniMatch.predict), coloured on the device')
    ap.add_argument('--scene', required=True, help='directory with color/, pose/ and intrinsic/')
    ap.add_argument('--out', required=True)
    ap.add_argument('--inference-size', type=int, nargs=2, default=None, metavar=('H', 'W'))
    ap.add_argument('--padding-factor', type=int, default=16)
    ap.add_argument('--min-depth', type=float, default=0.5)
    ap.add_argument('--max-depth', type=float, default=10.)
    ap.add_argument('--num-depth-candidates', type=int, default=64)
    ap.add_argument('--depth-from-argmax', action='store_true')
    ap.add_argument('--pred-bidir-depth', action='store_true')
    ap.add_argument('--scale-intrinsics', action='store_true', help='rescale the intrinsics with the resize (the reference does not)')
    ap.add_argument('--pairs-per-launch', type=int, default=None, metavar='N',
                    help='sequence mode: encode every frame once and match N pairs per launch (frames of one size)')
    ap.add_argument('--fuse-neighbours', action='store_true',
                    help='with --pairs-per-launch: the previous frame votes in every plane sweep as a second view (unlearned fusion; '
                         'not with --pred-bidir-depth)')
    ap.add_argument('--save-depth', action='store_true', help='write <stem>_depth.png: 16-bit millimetres')
    ap.add_argument('--consistency-check', action='store_true', help='write <stem>_occ.png: 255 where the neighbouring frames disagree')
    ap.add_argument('--save-ply', default=None, metavar='FILE', help='write the fused, filtered, coloured point cloud of the scene')
    ap.add_argument('--ply-stride', type=int, default=1, metavar='S', help='every S-th pixel of every row and column goes into the cloud')
    ap.add_argument('--save-tsdf-ply', default=None, metavar='FILE',
                    help='write the TSDF surface of the scene: the pixels --save-ply keeps, fused in one voxel grid')
    ap.add_argument('--save-tsdf-mesh', default=None, metavar='FILE',
                    help='write the triangle mesh of the TSDF volume of the scene (the options of --save-tsdf-ply apply)')
    ap.add_argument('--voxel-size', type=float, default=0.04, metavar='M', help='with --save-tsdf-ply: the edge of a voxel in metres')
    ap.add_argument('--tsdf-trunc', type=float, default=None, metavar='M', help='with --save-tsdf-ply: the truncation distance (default: 4 voxels)')
    ap.add_argument('--tsdf-min-weight', type=float, default=1., metavar='W',
                    help='with --save-tsdf-ply: the surface is taken between voxels of at least this accumulated weight')
    ap.add_argument('--min-views', type=int, default=1, help='neighbouring frames (of two) that must agree with a pixel to keep it')
    ap.add_argument('--px-thr', type=float, default=1.0, help='round-trip reprojection error a consistent pixel stays below (pixels)')
    ap.add_argument('--rel-thr', type=float, default=0.01, help='relative depth error a consistent pixel stays below')
    ap.add_argument('--save-confidence', action='store_true', help="write <stem>_conf.png: the plane sweep's max_prob, coloured")
    ap.add_argument('--min-confidence', type=float, default=None, metavar='P',
                    help='with --save-ply / --save-tsdf-ply: keep a pixel only where the probability mass around its best depth candidate is >= P '
                         '(with --pairs-per-launch and --pred-bidir-depth the last frame, seen backward, is not filtered on it)')
    ap.add_argument('--peak-radius', type=int, default=1, metavar='R', help='candidates each side of the best one that count as its peak')
    ap.add_argument('--model-config', default='gmdepth_s1', choices=[k for k, v in CONFIGS.items() if v[1].get('task') == 'depth'])
    ap.add_argument('--weights', default=None, help="checkpoint (the reference's: a state_dict, or {'model': state_dict}); "
                                                    'default: the seeded synthetic weights')
    ap.add_argument('--precision', default='exact', choices=['exact', 'fast'])
    args = ap.parse_args(argv)
    if args.fuse_neighbours and args.pairs_per_launch is None:
        ap.error('--fuse-neighbours needs --pairs-per-launch (it is an option of the sequence mode)')
    if args.fuse_neighbours and args.pred_bidir_depth:
        ap.error('--fuse-neighbours cannot be combined with --pred-bidir-depth (it replaces the backward prediction)')
    model, fwd_kw = load_model(args.model_config, args.weights, args.precision)
    n = run_depth(model, args.scene, args.out, fwd_kw, padding_factor=args.padding_factor, inference_size=args.inference_size,
                  min_depth=args.min_depth, max_depth=args.max_depth, num_depth_candidates=args.num_depth_candidates,
                  depth_from_argmax=args.depth_from_argmax, pred_bidir_depth=args.pred_bidir_depth,
                  scale_intrinsics=args.scale_intrinsics, pairs_per_launch=args.pairs_per_launch, save_depth=args.save_depth,
                  consistency_check=args.consistency_check, save_ply=args.save_ply, ply_stride=args.ply_stride, min_views=args.min_views,
                  px_thr=args.px_thr, rel_thr=args.rel_thr, save_confidence=args.save_confidence, min_confidence=args.min_confidence,
                  peak_radius=args.peak_radius, fuse_neighbours=args.fuse_neighbours, save_tsdf_ply=args.save_tsdf_ply, save_tsdf_mesh=args.save_tsdf_mesh,
                  voxel_size=args.voxel_size, tsdf_trunc=args.tsdf_trunc, tsdf_min_weight=args.tsdf_min_weight)
    print(f'{n} frames written to {args.out}')


if __name__ == '__main__':
    main()
