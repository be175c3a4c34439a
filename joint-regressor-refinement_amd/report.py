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

from . import _lib

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
