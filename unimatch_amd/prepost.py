"""The block the reference's evaluation scripts repeat around the model, built once (evaluate_flow.py:713-758,
evaluate_stereo.py:340-375 and :443-488, evaluate_depth.py:78-129): transpose tall inputs, pad or resize to the inference size, run
the forward, crop or resize the prediction back, rescale it.

  InferenceGeometry.padded(shape, mode, padding_factor)   the geometry of ``io.InputPadder`` (replicate padding, crop back)
  InferenceGeometry.resized(shape, inference_size)        bilinear resize, align_corners, and the per-kind rescale on the way back
  InferenceGeometry.nearest(shape, padding_factor)        resize to the next multiple of ``padding_factor``: the reference's default
                                                          when no inference size is given (evaluate_flow.py:719-723)
  geometry.prepare(*images, normalize=False)              images -> the model's input ``[B, 3, hp, wp]`` fp32
  geometry.restore(pred, kind='flow'|'disparity'|'depth') the prediction back at the images' size

Both take ``hflip=True``: a horizontal mirror as their LAST step, which is where the reference's stereo inference puts it (resize, then
``hflip``; resize back and rescale, then ``hflip``: evaluate_stereo.py:790-841), and ``out=``, a preallocated tensor to write into, so
that the doubled batch of a bidirectional prediction is built without a concatenation.  The mirror is part of the one launch and
equals ``torch.flip(<unflipped result>, [-1])`` bit for bit: the bilinear arithmetic is the mirrored column's.

CUDA tensors go to the HIP kernels (``um_image_prepare``, ``um_pred_restore``: one launch each, no synchronisation); a uint8
``[B, H, W, 3]`` batch, as a decoder delivers frames, is accepted as it is, so 3 bytes per pixel cross the bus instead of 12.  Host
tensors go to the restatement below, which is written out in the kernels' operation order -- ATen's bilinear arithmetic in fp32,
horizontal blends first, every product, sum and quotient rounded on its own -- and gives the same bits: the CPU tests pin it against
``F.interpolate`` and ``InputPadder``, the GPU tests pin the kernels against it.
"""
import numpy as np
import torch

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
KINDS = ('flow', 'disparity', 'depth')

_hip_ops = None


def _hip():
    global _hip_ops
    if _hip_ops is None:
        from .ops import HipOps            # raises when the HIP extension or the GPU is missing: there is no silent fallback
        _hip_ops = HipOps()
    return _hip_ops


def image_size(image):
    """``(H, W)`` of an image batch in either accepted layout: fp32 ``[B, 3, H, W]`` or uint8 ``[B, H, W, 3]``."""
    if image.dim() != 4:
        raise ValueError(f'expected a 4-dimensional image batch, got {tuple(image.shape)}')
    if image.dtype == torch.uint8:
        if image.shape[3] != 3:
            raise ValueError(f'expected uint8 frames [B, H, W, 3], got {tuple(image.shape)}')
        return int(image.shape[1]), int(image.shape[2])
    if image.shape[1] != 3:
        raise ValueError(f'expected images [B, 3, H, W], got {tuple(image.shape)}')
    return int(image.shape[2]), int(image.shape[3])


def _norm_constants(normalize):
    if normalize is None or normalize is False:
        return None, None
    if normalize is True:
        return IMAGENET_MEAN, IMAGENET_STD
    mean, std = normalize
    mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    if len(mean) != 3 or len(std) != 3 or any(s == 0 for s in std):
        raise ValueError('normalize is True, False or (mean, std) of three floats each with non-zero std')
    return mean, std


# ------------------------------------------------------------------ host restatement (the kernels' operation order)
def lerp_table(n_in, n_out):
    """``(i0, i1, l0, l1)`` of ATen's align_corners bilinear resize of ``n_in`` samples to ``n_out``, in fp32."""
    scale = float(np.float32(n_in - 1) / np.float32(n_out - 1)) if n_out > 1 else 0.0
    src = torch.arange(n_out, dtype=torch.float32) * scale
    i0 = src.to(torch.int64).clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    l1 = src - i0.float()
    return i0, i1, 1.0 - l1, l1


def resize_host(x, size):
    """Bilinear resize of ``x [..., h, w]`` fp32 to ``size``: the two horizontal blends, then the vertical one."""
    h, w = x.shape[-2:]
    y0, y1, ly0, ly1 = (t.to(x.device) for t in lerp_table(h, size[0]))
    x0, x1, lx0, lx1 = (t.to(x.device) for t in lerp_table(w, size[1]))
    r0, r1 = x.index_select(-2, y0), x.index_select(-2, y1)
    top = lx0 * r0.index_select(-1, x0) + lx1 * r0.index_select(-1, x1)
    bot = lx0 * r1.index_select(-1, x0) + lx1 * r1.index_select(-1, x1)
    return ly0[:, None] * top + ly1[:, None] * bot


def prepare_host(image, geom, mean=None, std=None, hflip=False):
    out = _prepare_host(image, geom, mean, std)
    return out.flip(-1).contiguous() if hflip else out


def _prepare_host(image, geom, mean=None, std=None):
    x = image.permute(0, 3, 1, 2).float() if image.dtype == torch.uint8 else image.float()
    if geom.transpose:
        x = x.transpose(-2, -1)
    if mean is not None:
        m = torch.tensor(mean, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
        s = torch.tensor(std, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
        x = (x / 255 - m) / s
    hp, wp = geom.size
    if geom.mode == 'resize':
        return resize_host(x, geom.size).contiguous()
    ih, iw = geom.image_size
    top, left = geom.crop
    iy = (torch.arange(hp, device=x.device) - top).clamp(0, ih - 1)
    ix = (torch.arange(wp, device=x.device) - left).clamp(0, iw - 1)
    return x.index_select(-2, iy).index_select(-1, ix).contiguous()


def restore_host(pred, geom, kind, hflip=False):
    out = _restore_host(pred, geom, kind)
    return out.flip(-1).contiguous() if hflip else out


def _restore_host(pred, geom, kind):
    ih, iw = geom.image_size
    hp, wp = geom.size
    if geom.mode == 'pad':
        top, left = geom.crop
        out = pred[..., top:top + ih, left:left + iw]
    else:
        out = resize_host(pred.float(), (ih, iw))
        if kind == 'flow':                                        # evaluate_flow.py:754-755: a multiply, then a divide
            out = torch.stack([out[:, 0] * float(iw) / float(wp), out[:, 1] * float(ih) / float(hp)], 1)
        elif kind == 'disparity':                                 # evaluate_stereo.py:375
            out = out * float(iw) / float(wp)
    if geom.transpose:                                            # evaluate_flow.py:757-758: the channels are not swapped
        out = out.transpose(-2, -1)
    return out.contiguous()


# ------------------------------------------------------------------ the geometry object
class InferenceGeometry:
    """How images of one shape are brought to the inference size and predictions brought back.

    ``shape``: the images' ``(..., H, W)`` (``image_size(x)`` for either layout).  ``transpose``: ``True`` / ``False``, or ``'auto'``:
    tall images (``H > W``) are transposed first, as evaluate_flow.py:713-717 does because the models are trained on wide frames; all
    sizes below are then those of the transposed frame (``image_size``).  Attributes: ``shape``, ``transpose``, ``image_size``,
    ``size`` (the inference size ``(hp, wp)``), ``mode`` (``'pad'`` / ``'resize'``), ``crop`` (``(top, left)`` of the image inside
    the padded frame; ``(0, 0)`` for a resize)."""

    def __init__(self, shape, size, mode, crop=(0, 0), transpose=False):
        self.shape = (int(shape[-2]), int(shape[-1]))
        self.transpose = self._resolve_transpose(self.shape, transpose)
        self.image_size = self.shape[::-1] if self.transpose else self.shape
        self.size = (int(size[0]), int(size[1]))
        if min(self.shape) < 1 or min(self.size) < 1:
            raise ValueError(f'empty geometry: images {self.shape}, inference size {self.size}')
        if mode not in ('pad', 'resize'):
            raise ValueError("mode must be 'pad' or 'resize'")
        if mode == 'resize' and self.size == self.image_size:     # the reference resizes (and rescales) only when the sizes differ
            mode, crop = 'pad', (0, 0)
        self.mode = mode
        self.crop = (int(crop[0]), int(crop[1])) if mode == 'pad' else (0, 0)
        top, left = self.crop
        ih, iw = self.image_size
        if mode == 'pad' and (top < 0 or left < 0 or top + ih > self.size[0] or left + iw > self.size[1]):
            raise ValueError(f'the image {ih}x{iw} at ({top}, {left}) leaves the padded size {self.size[0]}x{self.size[1]}')
        # F.pad order, as io.InputPadder keeps it: a pad-mode geometry (not transposed) can stand in for the padder of
        # metrics.*Metrics.update(..., padder=geometry), which then reads the padded prediction in place
        self._pad = [left, self.size[1] - iw - left, top, self.size[0] - ih - top] if mode == 'pad' else [0, 0, 0, 0]

    @staticmethod
    def _resolve_transpose(shape, transpose):
        if isinstance(transpose, str):
            if transpose != 'auto':
                raise ValueError("transpose must be 'auto', True or False")
            return shape[0] > shape[1]
        return bool(transpose)

    @classmethod
    def padded(cls, shape, mode='sintel', padding_factor=8, transpose=False):
        """Replicate padding to multiples of ``padding_factor`` with the pad amounts of ``io.InputPadder(shape, mode,
        padding_factor)``: ``mode='sintel'`` splits the vertical padding, any other mode puts it at the bottom."""
        hw = (int(shape[-2]), int(shape[-1]))
        ih, iw = hw[::-1] if cls._resolve_transpose(hw, transpose) else hw
        extra_h, extra_w = (-ih) % padding_factor, (-iw) % padding_factor
        top = extra_h // 2 if mode == 'sintel' else 0
        return cls(hw, (ih + extra_h, iw + extra_w), 'pad', (top, extra_w // 2), transpose)

    @classmethod
    def resized(cls, shape, inference_size, transpose=False):
        """Bilinear resize (align_corners) to ``inference_size = (hp, wp)``."""
        return cls(shape, inference_size, 'resize', (0, 0), transpose)

    @classmethod
    def nearest(cls, shape, padding_factor=8, transpose='auto'):
        """Resize to the next multiple of ``padding_factor`` in each dimension (evaluate_flow.py:719-723)."""
        hw = (int(shape[-2]), int(shape[-1]))
        ih, iw = hw[::-1] if cls._resolve_transpose(hw, transpose) else hw
        size = tuple(int(np.ceil(s / padding_factor)) * padding_factor for s in (ih, iw))
        return cls(hw, size, 'resize', (0, 0), transpose)

    def __repr__(self):
        return (f'InferenceGeometry(shape={self.shape}, size={self.size}, mode={self.mode!r}, crop={self.crop}, '
                f'transpose={self.transpose})')

    @property
    def identity(self):
        """Nothing to do to the geometry: same size, no transpose."""
        return self.mode == 'pad' and self.size == self.image_size and not self.transpose

    # -------------------------------------------------------------- images -> model input
    def prepare(self, *images, normalize=False, hflip=False, out=None):
        """Each of ``images`` (fp32 ``[B, 3, H, W]`` or uint8 ``[B, H, W, 3]``) as the model's input ``[B, 3, hp, wp]`` fp32, in a
        list.  ``normalize``: ``False`` (flow: the model normalises raw 0..255 values itself), ``True`` (``(x / 255 - mean) / std``
        with the ImageNet constants, what the stereo and depth loaders do on the host) or ``(mean, std)``.  An fp32 batch that
        needs nothing is returned as it is.  ``hflip``: mirrored horizontally after everything else.  ``out``: a preallocated
        contiguous fp32 ``[B, 3, hp, wp]`` tensor per image (one tensor for one image, else a sequence; a batch slice of a larger
        tensor qualifies) that receives the result and is returned in its place."""
        mean, std = _norm_constants(normalize)
        if out is None:
            dsts = [None] * len(images)
        else:
            dsts = [out] if torch.is_tensor(out) else list(out)
            if len(dsts) != len(images):
                raise ValueError(f'out: {len(dsts)} tensors for {len(images)} images')
        out = []
        for image, dst in zip(images, dsts):
            if image_size(image) != self.shape:
                raise ValueError(f'this geometry is for images of {self.shape[0]}x{self.shape[1]}, got {tuple(image.shape)} {image.dtype}')
            if image.dtype != torch.uint8 and not image.is_floating_point():
                raise ValueError(f'expected float or uint8 images, got {image.dtype}')
            if dst is not None and (tuple(dst.shape) != (image.shape[0], 3) + self.size or dst.dtype != torch.float32
                                    or dst.device != image.device or not dst.is_contiguous()):
                raise ValueError(f'out must be a contiguous float32 {(image.shape[0], 3) + self.size} tensor on {image.device}, got '
                                 f'{tuple(dst.shape)} {dst.dtype} {dst.device}')
            if self.identity and mean is None and image.dtype == torch.float32 and not hflip and dst is None:
                out.append(image)
            elif image.is_cuda:
                with torch.cuda.device(image.device):
                    src = image if image.dtype == torch.uint8 else image.float()
                    out.append(_hip().image_prepare(src, self.size, self.mode, self.crop, self.transpose, mean, std, hflip=hflip, out=dst))
            else:
                res = prepare_host(image, self, mean, std, hflip)
                out.append(res if dst is None else dst.copy_(res))
        return out

    # -------------------------------------------------------------- prediction -> the images' frame
    def restore(self, pred, kind='flow', hflip=False, out=None):
        """The prediction ``[B, C, hp, wp]`` (or ``[B, hp, wp]``, as the model returns disparities and depths) at the images' size:
        cropped, or resized and rescaled -- flow ``u * W / wp`` and ``v * H / hp``, disparity ``* W / wp``, depth not at all
        (evaluate_depth.py:131) -- and transposed back.  The reference does not swap the flow channels when it transposes back
        (evaluate_flow.py:757-758) and neither does this: channel 0 stays the displacement along the transposed frame's x.
        ``hflip``: mirrored horizontally after everything else.  ``out``: a preallocated contiguous fp32 tensor of the result's shape
        that receives it."""
        if kind not in KINDS:
            raise ValueError(f'kind must be one of {KINDS}, got {kind!r}')
        squeeze = pred.dim() == 3
        p = pred.unsqueeze(1) if squeeze else pred
        channels = 2 if kind == 'flow' else 1
        if p.dim() != 4 or p.shape[1] != channels or tuple(p.shape[-2:]) != self.size:
            raise ValueError(f'expected a {kind} prediction [B, {channels}, {self.size[0]}, {self.size[1]}]'
                             f"{' or [B, hp, wp]' if channels == 1 else ''}, got {tuple(pred.shape)}")
        if self.identity and not hflip and out is None:
            return pred
        want = tuple(pred.shape[:-2]) + self.shape
        if out is not None and (tuple(out.shape) != want or out.dtype != torch.float32 or out.device != pred.device
                                or not out.is_contiguous()):
            raise ValueError(f'out must be a contiguous float32 {want} tensor on {pred.device}, got {tuple(out.shape)} {out.dtype} '
                             f'{out.device}')
        dst = out.unsqueeze(1) if (out is not None and squeeze) else out
        if p.is_cuda:
            with torch.cuda.device(p.device):
                res = _hip().pred_restore(p.float(), self.shape, self.mode, self.crop, kind, self.transpose, hflip=hflip, out=dst)
        else:
            res = restore_host(p.float(), self, kind, hflip)
            res = res if dst is None else dst.copy_(res)
        return res.squeeze(1) if squeeze else res

    def scaled_intrinsics(self, intrinsics):
        """Opt-in, for depth resizes: ``intrinsics [..., 3, 3]`` with rows 0 and 1 multiplied by ``(wp - 1) / (W - 1)`` and ``(hp -
        1) / (H - 1)``, the pixel mapping of an align_corners resize.  The reference leaves the intrinsics untouched when it resizes
        (evaluate_depth.py:81-86), and so does every default path here."""
        if self.transpose:
            raise ValueError('scaled_intrinsics: a transposed geometry has no intrinsics convention')
        if self.mode == 'pad' and self.crop != (0, 0):
            raise ValueError('scaled_intrinsics is for resizes: padding at an offset shifts the principal point instead')
        (h, w), (hp, wp) = self.image_size, self.size
        fx = (wp - 1) / (w - 1) if w > 1 else 1.0
        fy = (hp - 1) / (h - 1) if h > 1 else 1.0
        scale = torch.tensor([fx, fy, 1.0], dtype=intrinsics.dtype, device=intrinsics.device).view(3, 1)
        return intrinsics * scale


def geometry_for(shape, inference_size=None, padding_factor=8, pad_mode='kitti', transpose=False):
    """The geometry the reference's validation loops choose: padding when no inference size is given, else a resize."""
    if inference_size is None:
        return InferenceGeometry.padded(shape, pad_mode, padding_factor, transpose)
    return InferenceGeometry.resized(shape, inference_size, transpose)
