"""The fit report: how well the refined meshes cover their masks, and pictures of it.

The reference renders the mesh before and after its 100 iterations and hands the render to `viz()`
(/root/reference/scripts/optimize.py:204-218, :268-274, viz at :28-74): `render > 0.5`, `mask_rcnn > 0.8`, the map
`mask + render == 1` with the 2-D joints scattered over it, one PNG per pose.  Here the comparison (jrr_silhouette_compare) and the
compositing (jrr_fit_overlay) run on the device over the whole batch; only the PNG encoder is host code, standard library only.
"""
from __future__ import annotations

import struct
import zlib
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, dist as jdist, engine as _engine

THR_RENDER, THR_MASK = 0.5, 0.8        # scripts/optimize.py:35,41


def _planes(t: torch.Tensor, name: str) -> torch.Tensor:
    """(B,S,S) or (B,1,S,S) float32 device tensor -> contiguous (B,h,w)"""
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3 or t.dtype != torch.float32 or not t.is_cuda:
        raise ValueError(f'{name}: expected a float32 device tensor (B,h,w) or (B,1,h,w), got {tuple(t.shape)} {t.dtype} on {t.device}')
    return t.contiguous()


def _pair(alpha: torch.Tensor, mask: torch.Tensor):
    alpha, mask = _planes(alpha, 'alpha'), _planes(mask, 'mask')
    if alpha.shape != mask.shape or alpha.device != mask.device:
        raise ValueError(f'alpha {tuple(alpha.shape)} on {alpha.device} and mask {tuple(mask.shape)} on {mask.device} differ')
    return alpha, mask


def silhouette_compare(alpha: torch.Tensor, mask: torch.Tensor, thr_render: float = THR_RENDER, thr_mask: float = THR_MASK) -> torch.Tensor:
    """per pose the pixel counts {r & m, r | m, r, m} of r = alpha > thr_render, m = mask > thr_mask (strict, fp32): int32 (B,4)"""
    alpha, mask = _pair(alpha, mask)
    B, h, w = alpha.shape
    counts = torch.empty(B, 4, dtype=torch.int32, device=alpha.device)
    _lib.check(_lib.load().jrr_silhouette_compare(_lib.ptr(alpha), _lib.ptr(mask), B, h, w, float(thr_render), float(thr_mask),
                                                  _lib.ptr(counts), _lib.stream_ptr(alpha.device)), 'silhouette_compare')
    return counts


def iou_from_counts(counts: torch.Tensor) -> torch.Tensor:
    """intersection / union in float64; 1.0 where the union is empty (both silhouettes are empty and agree)"""
    inter, union = counts[:, 0].double(), counts[:, 1].double()
    return torch.where(union > 0, inter / union.clamp(min=1), torch.ones_like(union))


def silhouette_iou(alpha: torch.Tensor, mask: torch.Tensor, thr_render: float = THR_RENDER, thr_mask: float = THR_MASK) -> torch.Tensor:
    """intersection over union of the two thresholded silhouettes per pose: float64 (B)"""
    return iou_from_counts(silhouette_compare(alpha, mask, thr_render, thr_mask))


def fit_overlay(alpha: torch.Tensor, mask: torch.Tensor, image: Optional[torch.Tensor] = None, normalize=None,
                joints2d: Sequence[torch.Tensor] = (), radius: float = 2.0, thr_render: float = THR_RENDER,
                thr_mask: float = THR_MASK, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The picture of every pose: uint8 (B,S,S,3).  image (B,3,S,S) is the background (black without one); normalize = (mean, std)
    says it is the normalised SPIN crop and is undone; render only red, mask only blue, both green, each averaged with the
    background; joints2d: up to three (B,17,2) sets in the crop's pixel frame, drawn as discs of `radius` pixels in green (set 0: the
    target), yellow, magenta, a later set over an earlier one.  `out`: a caller-owned contiguous uint8 (B,S,S,3) tensor to write into."""
    alpha, mask = _pair(alpha, mask)
    B, S, S2 = alpha.shape
    dev = alpha.device
    if S != S2:
        raise ValueError(f'fit_overlay: square images, got {S} x {S2}')
    if image is not None:
        if tuple(image.shape) != (B, 3, S, S) or image.dtype != torch.float32 or image.device != dev:
            raise ValueError(f'image: expected float32 {(B, 3, S, S)} on {dev}, got {tuple(image.shape)} {image.dtype} on {image.device}')
        image = image.contiguous()
    mean = std = None
    if normalize is not None:
        if image is None:
            raise ValueError('fit_overlay: normalize without an image')
        mean = torch.tensor(normalize[0], dtype=torch.float32, device=dev)
        std = torch.tensor(normalize[1], dtype=torch.float32, device=dev)
        if mean.shape != (3,) or std.shape != (3,):
            raise ValueError('fit_overlay: normalize = (mean, std) of 3 values each')
    sets = list(joints2d)
    if len(sets) > 3:
        raise ValueError('fit_overlay: at most three joint sets')
    j2d = None
    if sets:
        for s in sets:
            if tuple(s.shape) != (B, 17, 2):
                raise ValueError(f'joints2d: expected (B,17,2) = {(B, 17, 2)}, got {tuple(s.shape)}')
        j2d = torch.stack([s.to(dev, torch.float32) for s in sets]).contiguous()
    if out is None:
        out = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != (B, S, S, 3) or out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous():
        raise ValueError(f'out: expected a contiguous uint8 {(B, S, S, 3)} on {dev}')
    _lib.check(_lib.load().jrr_fit_overlay(_lib.ptr(alpha), _lib.ptr(mask), _lib.ptr(image), _lib.ptr(mean), _lib.ptr(std), _lib.ptr(j2d),
                                           len(sets), B, S, float(thr_render), float(thr_mask), float(radius), _lib.ptr(out),
                                           _lib.stream_ptr(dev)), 'fit_overlay')
    return out


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)


def write_png(path: str, rgb) -> None:
    """an (H,W,3) uint8 array or tensor as an 8-bit RGB PNG, non-interlaced, filter 0 on every scanline (zlib and struct only)"""
    if torch.is_tensor(rgb):
        rgb = rgb.detach().cpu().numpy()
    rgb = np.ascontiguousarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.dtype != np.uint8 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError(f'write_png: expected uint8 (H,W,3), got {rgb.dtype} {rgb.shape}')
    h, w = rgb.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)           # filter byte 0 + the scanline
    rows[:, 1:] = rgb.reshape(h, 3 * w)
    png = (b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0))
           + _chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + _chunk(b'IEND', b''))
    with open(path, 'wb') as f:
        f.write(png)


class FitReport:
    """`--fit_report DIR` of one run (scripts/optimize.py:204-218 before the loop, :268-274 after it, viz() at :28-74): per outer batch and
    shard the mesh is rendered with the poses as they stand, compared with the batch's mask, the regressed joints are projected.
    `before` and `after` each run a forward of their own on the batch's engine, so each sits where no later call reads the engine's
    most recent forward.  They take the driver's batch object: its engine, mask, poses, shard bounds and global batch."""

    def __init__(self, directory: str, n_images: int):
        self.directory, self.n_images = directory, int(n_images)
        self.last = None           # the run's `fit_report` return value: per-pose IoU of the last batch's shard

    def before(self, b):
        self.gt_j2d = b.gt_j2d     # the loop's own 2-D target (--reprojection), else the dataset's, else none
        if self.gt_j2d is None and 'gt_j2d' in b.full:
            self.gt_j2d = b.full['gt_j2d'][b.lo:b.hi].to(b.sil_mask.device).float().contiguous()
        self.n = max(0, min(self.n_images, b.eng.batch))
        self.sums = torch.zeros(4, dtype=torch.float64, device=b.sil_mask.device)     # IoU before / after, pixel error before / after
        self.iou, self.kept = {}, {}
        self._render('before', b)

    def after(self, b):
        self._render('after', b)
        jdist.all_reduce_sum_(self.sums)                                              # the one extra (32-byte) collective of --fit_report
        self._write(b)

    def record(self, b) -> dict:
        """the record's four fields (means over the GLOBAL batch); reads the sums back"""
        fs = self.sums.cpu().numpy() / b.B_global
        px = (fs[2], fs[3]) if self.gt_j2d is not None else (None, None)
        self.last = {'iou_before': self.iou['before'].cpu().numpy(), 'iou_after': self.iou['after'].cpu().numpy(), 'shard': (b.lo, b.hi)}
        return {'silhouette_iou_before': fs[0], 'silhouette_iou_after': fs[1], 'j2d_error_px_before': px[0], 'j2d_error_px_after': px[1]}

    def _render(self, when: str, b):
        k = ('before', 'after').index(when)
        joints, verts = b.eng.find_joints_forward(b.betas, x6d=b.x6d, return_verts=True)
        alpha = b.eng.silhouette_forward(verts, b.cam)
        j2d = _engine.project_joints(joints, b.cam)
        self.iou[when] = iou_from_counts(silhouette_compare(alpha, b.sil_mask))
        self.sums[k] = self.iou[when].sum()
        if self.gt_j2d is not None:
            self.sums[2 + k] = (j2d - self.gt_j2d).norm(dim=-1).mean(-1).sum().double()
        self.kept[when] = (alpha[:self.n].clone(), j2d[:self.n].clone())

    def _write(self, b):
        """overlays of the shard's first poses: target joints green, initial yellow, refined magenta (the last on `after` only); under
        `--image_masks` over the 224 crop the SPIN network saw, de-normalised"""
        import os
        from .data import SPIN_NORMALIZE
        if self.n == 0:
            return
        os.makedirs(self.directory, exist_ok=True)
        n = self.n
        image = b.images['spin_image'][:n] if b.images is not None else None
        target = self.gt_j2d[:n] if self.gt_j2d is not None else torch.full_like(self.kept['before'][1], float('nan'))
        sets = {'before': [target, self.kept['before'][1]], 'after': [target, self.kept['before'][1], self.kept['after'][1]]}
        for when in ('before', 'after'):
            rgb = fit_overlay(self.kept[when][0], b.sil_mask[:n], image=image, normalize=SPIN_NORMALIZE if image is not None else None,
                              joints2d=sets[when]).cpu().numpy()
            for i in range(n):
                write_png(os.path.join(self.directory, f'b{b.it:04d}_p{b.lo + i:05d}_{when}.png'), rgb[i])
