"""Human3.6M samples in the reference's on-disk layout: precomputed tensors and the image pipeline.

The reference's `data_set(set)` (/root/reference/scripts/data.py:28-163) reads, per split directory
`data/human3.6m/precomputed_{train,val}/`:
    bboxes.pt  betas.pt  estimated_translation.pt  gt_j2d.pt  gt_j3d.pt  intrinsics.pt  orient.pt  pose.pt
    images.pkl  pixel_annotations.pkl
and, per sample, a JPEG frame + a Mask-RCNN mask; the frame is cropped twice with a similarity-warp image sampler
(data.py:110-128, 220-271: 224 px for the SPIN network, 256 px for `image`).  Human3.6M is licensed and absent.

Tensor part (always):
  * the same file names and split directories,
  * the crop parameters of find_crop (data.py:220-247) computed from the bounding boxes alone (`crop_params`),
  * gt_j2d repositioned into the 224-crop pixel frame exactly as data.py:134-138.
  `data_set(set, root)` WITHOUT a frame source yields the tensor-valued keys only (the reference's minus 'image', 'spin_image',
  'mask_rcnn', 'valid').

Image part (`data_set(set, root, frames=<frame source>)`): the reference's full key set (data.py:140-158).
  * `find_crop` / `crop_intrinsics` / `resize_intrinsics` (data.py:220-271, 385-449) in pure torch for DataLoader workers; the
    warp has no rotation (theta = 0), so the bilinear sampling is separable and evaluated from per-row / per-column taps.
  * frame sources: `ArrayFrameSource` (arrays in memory or one .npy pair per sample) and `FileFrameSource` (paths from images.pkl,
    decoded with PIL).  The reference's `--compute_canada` HDF5 branch (data.py:92-107) needs h5py and is not built.
  * `crop_batch`: the device route for whole batches -- uint8 pixels up, ONE launch of the HIP kernel k_image_crop for both crop
    sizes and one of k_mask_prepare (csrc/image.hip, include/jrr.h).  Only the rows and columns a crop can touch are uploaded (a
    region of interest per sample); the kernel raises a status word, and crop_batch an exception, if a tap falls outside it.
"""
from __future__ import annotations

import os
import pickle
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset

TENSOR_FILES = ['bboxes', 'betas', 'estimated_translation', 'gt_j2d', 'gt_j3d', 'intrinsics', 'orient', 'pose']
IMG_RES = 1000           # frames are cut to [:1000, :1000] (scripts/constants.py IMG_RES, data.py:111-112)
SPIN_SIZE, IMAGE_SIZE = 224, 256
REFERENCE_KEYS = ('bboxes', 'betas', 'cam', 'gt_j2d', 'gt_j3d', 'valid', 'mask_rcnn', 'image', 'spin_image', 'intrinsics', 'orient',
                  'pose', 'inc_gt')
SPIN_NORMALIZE = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))     # scripts/optimize.py:141-142


def crop_params(bboxes: torch.Tensor):
    """find_crop's geometry (data.py:222-247): bboxes (N,4) = (min_y, min_x, max_y, max_x) in the 1000-px frame
    -> (min_x, min_y, scale) of the square crop; scale = half side in units of 500 px."""
    min_x, max_x = (bboxes[:, 1] - 500) / 500, (bboxes[:, 3] - 500) / 500
    min_y, max_y = (bboxes[:, 0] - 500) / 500, (bboxes[:, 2] - 500) / 500
    average_x, average_y = (min_x + max_x) / 2, (min_y + max_y) / 2
    scale = torch.maximum(max_x - min_x, max_y - min_y) / 2
    return (average_x - scale) * 500 + 500, (average_y - scale) * 500 + 500, scale


def reposition_j2d(gt_j2d: torch.Tensor, bboxes: torch.Tensor) -> torch.Tensor:
    """data.py:134-138: 2-D joints (N,17,2) in the 1000-px frame -> the 224-crop pixel frame."""
    min_x, min_y, scale = crop_params(bboxes)
    out = gt_j2d.clone()
    out[..., 0] -= min_x[:, None]
    out[..., 1] -= min_y[:, None]
    out /= scale[:, None, None]
    out /= 1000 / 224
    return out


# ---- the crop (data.py:220-271) --------------------------------------------------------------------------------------------
def _crop_centres(bboxes: torch.Tensor):
    """bbox centre (x, y) in units of 500 px about 500 and the half side `scale` (data.py:228-244)"""
    min_x, max_x = (bboxes[:, 1] - 500) / 500, (bboxes[:, 3] - 500) / 500
    min_y, max_y = (bboxes[:, 0] - 500) / 500, (bboxes[:, 2] - 500) / 500
    return (min_x + max_x) / 2, (min_y + max_y) / 2, torch.maximum(max_x - min_x, max_y - min_y) / 2


def linspace_pm1(n: int, dtype=torch.float32) -> torch.Tensor:
    """linspace(-1, 1, n) by torch's scalar formula -- start + step * i below the middle, end - step * (n - 1 - i) from it on, every
    operation rounded once.  torch.linspace itself fills whole SIMD vectors from one base value, so its last bit depends on the
    host's vector width; the host code and the kernel need ONE definition to agree on every tap (the region of interest is exact)."""
    i = torch.arange(n, dtype=dtype)
    step = torch.tensor(2.0, dtype=dtype) / (n - 1)
    return torch.where(i < n // 2, -1 + step * i, 1 - step * (n - 1 - i))


def axis_taps(scale: torch.Tensor, centre: torch.Tensor, n: int, extent: int):
    """The two bilinear taps of every output index along ONE axis: (i0 (B,n) int64, w0, w1 (B,n)); the taps are pixels i0 and i0 + 1.

    The similarity matrix of data.py:255-261 with theta = 0 is [[s, 0, s (ax / s)], [0, s, s (ay / s)], [0, 0, 1]]; output index j sits at
    linspace(-1, 1, n)[j] (sampling_helper.py:46-49), the homogeneous divide is by 1 + 1e-8 = 1 in the arithmetic's precision
    (sampling_helper.py:62), and grid_sample (bilinear, align_corners=False) reads position ((g + 1) * extent - 1) / 2.  A tap outside
    [0, extent) has weight 0 (zero padding); a position that is not finite (scale = 0) has both weights 0, which is the reference's
    "nan value in warped image! set to zeros" (sampling_helper.py:36-38).  i0 is clamped to [-2, extent].  Every operation is one
    rounding in the dtype of `scale`, in this order: csrc/image.hip repeats it."""
    lin = linspace_pm1(n, scale.dtype)
    g =scale[:, None] * lin[None, :] + (scale * (centre / scale))[:, None]
    pos = ((g + 1) * extent - 1) / 2
    finite = torch.isfinite(pos)
    f = torch.floor(pos)
    w1, w0 = pos - f, (f + 1) - pos
    i0 = torch.where(finite, f.clamp(-2, extent), torch.full_like(f, -2)).long()
    zero = torch.zeros_like(pos)
    w0 = torch.where(finite & (i0 >= 0) & (i0 < extent), w0, zero)
    w1 = torch.where(finite & (i0 + 1 >= 0) & (i0 + 1 < extent), w1, zero)
    return i0, w0, w1


def _tap_range(i0, w0, w1):
    """[lo, hi) pixel range of the taps with non-zero weight along one axis, per sample; (0, 0) when there is none"""
    big = torch.iinfo(torch.int64).max
    lo = torch.minimum(torch.where(w0 != 0, i0, big).amin(1), torch.where(w1 != 0, i0 + 1, big).amin(1))
    hi = torch.maximum(torch.where(w0 != 0, i0, -1).amax(1), torch.where(w1 != 0, i0 + 1, -1).amax(1)) + 1
    empty = hi <= 0
    return torch.where(empty, 0, lo), torch.where(empty, 0, hi)


def crop_roi(bboxes: torch.Tensor, height: int, width: int, sizes: Sequence[int] = (SPIN_SIZE, IMAGE_SIZE)) -> torch.Tensor:
    """(B,4) int64 (y0, x0, h, w): per sample the smallest block of the height x width frame that holds every tap of non-zero weight
    of the crops at `sizes`; (0, 0, 0, 0) for a crop that reads nothing (wholly outside, zero size)."""
    ax, ay, scale = _crop_centres(bboxes.float())
    ylo, yhi = _tap_range(*(torch.cat(t, 1) for t in zip(*(axis_taps(scale, ay, n, height) for n in sizes))))
    xlo, xhi = _tap_range(*(torch.cat(t, 1) for t in zip(*(axis_taps(scale, ax, n, width) for n in sizes))))
    h, w = yhi - ylo, xhi - xlo
    none = (h <= 0) | (w <= 0)
    z = torch.zeros_like(h)
    return torch.stack([torch.where(none, z, ylo), torch.where(none, z, xlo), torch.where(none, z, h), torch.where(none, z, w)], 1)


def crop_intrinsics(intrinsics, height, width, crop_ci, crop_cj):
    """data.py:385-410: the camera matrix (B,3,3) of a height x width window centred at row crop_ci, column crop_cj: the principal
    point moves with the window."""
    out = intrinsics.clone()
    out[:, 0, 2] = intrinsics[:, 0, 2] + (width - 1) / 2 - crop_cj
    out[:, 1, 2] = intrinsics[:, 1, 2] + (height - 1) / 2 - crop_ci
    return out


def resize_intrinsics(intrinsics, height, width, scale):
    """data.py:413-449: the camera matrix of the height x width image resized by `scale`: focal lengths scale, the principal point
    keeps its offset from the image centre, scaled."""
    off_x = intrinsics[:, 0, 2] - (width - 1) / 2
    off_y = intrinsics[:, 1, 2] - (height - 1) / 2
    out = intrinsics.clone()
    out[:, 0, 2] = (scale * width - 1) / 2 + scale * off_x
    out[:, 1, 2] = (scale * height - 1) / 2 + scale * off_y
    out[:, 0, 0] = scale * intrinsics[:, 0, 0]
    out[:, 1, 1] = scale * intrinsics[:, 1, 1]
    return out


def _crop_geometry(bboxes, intrinsics, img_size):
    """(min_x, min_y, scale, intrinsics of the crop) of data.py:246-247,258-269"""
    ax, ay, scale = _crop_centres(bboxes)
    min_x, min_y = (ax - scale) * 500 + 500, (ay - scale) * 500 + 500
    k = crop_intrinsics(intrinsics, 1000 * scale, 1000 * scale, ay * 500 + 500, ax * 500 + 500)
    k = resize_intrinsics(k, 1000 * scale, 1000 * scale, img_size / (scale * 1000))
    return min_x, min_y, scale, k


def find_crop(image, bboxes, intrinsics, img_size=256, roi=None):
    """data.py:220-271.  image (3,H,W) or (B,3,H,W) float in [0, 1]; bboxes (B,4) = (min_y, min_x, max_y, max_x) in the 1000-unit frame
    convention whatever H and W are; intrinsics (B,3,3) -> (crop (B,3,img_size,img_size), min_x, min_y, scale, intrinsics).

    roi = (y0, x0, H, W) (ints, or (B,4) for a batch): `image` is only the block [y0 : y0 + h, x0 : x0 + w] of an H x W frame.  A tap of
    non-zero weight inside the frame but outside the block is an error (the device kernel's status word, here a ValueError)."""
    if image.dim() == 3:
        image = image[None]
    B = bboxes.shape[0]
    if image.shape[0] != B:
        raise ValueError(f'{image.shape[0]} images for {B} bounding boxes')
    bboxes = bboxes.to(image.dtype)
    h, w = image.shape[-2:]
    if roi is None:
        roi = torch.tensor([[0, 0, h, w]] * B)
    roi = torch.as_tensor(roi).reshape(-1, 4).expand(B, 4)
    ax, ay, scale = _crop_centres(bboxes)
    out = image.new_zeros(B, image.shape[1], img_size, img_size)
    for b in range(B):
        y0, x0, H, W = (int(v) for v in roi[b])
        iy, wy0, wy1 = (t[0] for t in axis_taps(scale[b:b + 1], ay[b:b + 1], img_size, H))
        ix, wx0, wx1 = (t[0] for t in axis_taps(scale[b:b + 1], ax[b:b + 1], img_size, W))
        for i0, a0, a1, off, ext, what in ((iy, wy0, wy1, y0, h, 'row'), (ix, wx0, wx1, x0, w, 'column')):
            lost = ((a0 != 0) & ((i0 < off) | (i0 >= off + ext))) | ((a1 != 0) & ((i0 + 1 < off) | (i0 + 1 >= off + ext)))
            if lost.any():
                raise ValueError(f'find_crop: sample {b}: a {what} tap of non-zero weight lies outside the region of interest {(y0, x0, h, w)}')
        if h == 0 or w == 0:
            continue
        r0, r1 = (iy - y0).clamp(0, h - 1), (iy + 1 - y0).clamp(0, h - 1)
        c0, c1 = (ix - x0).clamp(0, w - 1), (ix + 1 - x0).clamp(0, w - 1)
        img = image[b]
        top, bottom = img[:, r0], img[:, r1]
        # grid_sample's sum: north-west, north-east, south-west, south-east, each weight the product of its two factors
        acc = top[:, :, c0] * (wy0[:, None] * wx0[None, :]) + top[:, :, c1] * (wy0[:, None] * wx1[None, :])
        acc = acc + bottom[:, :, c0] * (wy1[:, None] * wx0[None, :])
        out[b] = acc + bottom[:, :, c1] * (wy1[:, None] * wx1[None, :])
    min_x, min_y, scale, k = _crop_geometry(bboxes, intrinsics.to(image.dtype), img_size)
    return out, min_x, min_y, scale, k


# ---- frame sources ---------------------------------------------------------------------------------------------------------
class ArrayFrameSource:
    """read(index) -> (frame uint8 (H,W,3), mask uint8 (h,w)) from arrays in memory, or from a directory with one
    `frame_%06d.npy` / `mask_%06d.npy` pair per sample."""

    def __init__(self, frames=None, masks=None, directory: Optional[str] = None):
        if (directory is None) == (frames is None):
            raise ValueError('ArrayFrameSource takes either arrays or a directory')
        self.frames, self.masks, self.directory = frames, masks, directory

    @staticmethod
    def present(directory: str) -> bool:
        return os.path.exists(os.path.join(directory, 'frame_000000.npy'))

    def read(self, index: int):
        if self.directory is not None:
            frame = np.load(os.path.join(self.directory, f'frame_{index:06d}.npy'))
            mask = np.load(os.path.join(self.directory, f'mask_{index:06d}.npy'))
        else:
            frame, mask = self.frames[index], self.masks[index]
        return _checked(np.asarray(frame), np.asarray(mask), index)


class FileFrameSource:
    """read(index) from the image files listed in images.pkl (data.py:60-61,110); the mask's path is the frame's with
    `imageSequence` replaced by `maskSequence` (data.py:115-118).  Decoded with PIL."""

    def __init__(self, location: str):
        with open(os.path.join(location, 'images.pkl'), 'rb') as f:
            self.images = [str(p) for p in pickle.load(f)]

    def read(self, index: int):
        from PIL import Image
        path = self.images[index]
        head, sep, tail = path.partition('imageSequence')
        if not sep:
            raise ValueError(f'sample {index}: {path} has no imageSequence component to derive the mask path from')
        frame = np.asarray(Image.open(path).convert('RGB'))
        mask = np.asarray(Image.open(f'{head}maskSequence{tail}').convert('L'))
        return _checked(frame, mask, index)


def _checked(frame, mask, index):
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError(f'sample {index}: frame must be uint8 (H,W,3), got {frame.dtype} {frame.shape}')
    if mask.dtype != np.uint8 or mask.ndim != 2:
        raise ValueError(f'sample {index}: mask must be uint8 (h,w), got {mask.dtype} {mask.shape}')
    return frame, mask


def split_location(set: str, root: str) -> str:
    return os.path.join(root, 'precomputed_train' if set == 'train' else 'precomputed_val')


def split_image_paths(location: str):
    """the frame paths of images.pkl (data.py:60-61), one per sample, or None when the split directory has no such file: what the
    evaluation report groups by (eval_report.group_of)"""
    p = os.path.join(location, 'images.pkl')
    if not os.path.isfile(p):
        return None
    with open(p, 'rb') as f:
        return [str(x) for x in pickle.load(f)]


def frame_source_for(location: str):
    """the .npy source when the split directory holds one, else the image files of images.pkl"""
    return ArrayFrameSource(directory=location) if ArrayFrameSource.present(location) else FileFrameSource(location)


class data_set(Dataset):
    """data_set("train" | "validation"): samples of the reference's dataset.  frames=None: the nine tensor-valued keys.  With a frame
    source: the reference's thirteen keys, crops made on the host by find_crop (device_crops=False), or the nine keys plus 'index'
    for a caller that crops whole batches on the device with crop_batch (device_crops=True).  with_index=True adds 'index' to any of
    them (the refined-pose table is keyed by it)."""

    def __init__(self, set: str, root: str = 'data/human3.6m', frames=None, device_crops: bool = False, compute_canada: bool = False,
                 with_index: bool = False):
        if compute_canada:
            raise NotImplementedError('the HDF5 branch of the reference (--compute_canada, scripts/data.py:92-107) needs h5py and is not built')
        location = split_location(set, root)
        missing = [f for f in TENSOR_FILES if not os.path.exists(os.path.join(location, f + '.pt'))]
        if missing:
            raise FileNotFoundError(f'{location}: missing {missing} (Human3.6M precomputed tensors are not shipped; '
                                    f'use the synthetic batches of smpl_model.synthetic_batch instead)')
        for f in TENSOR_FILES:
            setattr(self, f, torch.load(os.path.join(location, f + '.pt'), map_location='cpu').float())
        n = self.gt_j3d.shape[0]
        for f in TENSOR_FILES:
            if getattr(self, f).shape[0] != n:
                raise ValueError(f'{f}.pt has {getattr(self, f).shape[0]} rows, gt_j3d.pt has {n}')
        self.inc_gt = torch.ones(n, dtype=torch.bool)
        self.gt_j2d_crop = reposition_j2d(self.gt_j2d, self.bboxes)
        self.frames, self.device_crops, self.with_index = frames, device_crops, with_index

    def __len__(self):
        return self.gt_j3d.shape[0]

    def __getitem__(self, index) -> Dict[str, torch.Tensor]:
        out = {'bboxes': self.bboxes[index], 'betas': self.betas[index], 'cam': self.estimated_translation[index],
               'gt_j2d': self.gt_j2d_crop[index], 'gt_j3d': self.gt_j3d[index], 'intrinsics': self.intrinsics[index],
               'orient': self.orient[index], 'pose': self.pose[index], 'inc_gt': self.inc_gt[index]}
        if self.with_index:                                                                  # where the sample sits in the split
            out['index'] = torch.tensor(int(index))
        if self.frames is None:
            return out
        if self.device_crops:
            out['index'] = torch.tensor(int(index))
            return out
        frame, mask = self.frames.read(int(index))                                           # data.py:110-121
        image = torch.from_numpy(np.ascontiguousarray(frame)).permute(2, 0, 1)[:, :IMG_RES, :IMG_RES].float() / 255.0
        mask_rcnn = torch.from_numpy(np.ascontiguousarray(mask)).float().unsqueeze(0) / 255.0
        bbox, k = self.bboxes[index][None], self.intrinsics[index][None]
        out['spin_image'] = find_crop(image, bbox, k, img_size=SPIN_SIZE)[0][0]              # data.py:123-124
        crop, _, _, _, k256 = find_crop(image, bbox, k, img_size=IMAGE_SIZE)                 # data.py:126-127
        out['valid'] = mask_rcnn[0, 0, 0] != 0                                               # data.py:130: BEFORE the corner is zeroed
        mask_rcnn[:, :2, :2] = 0                                                             # data.py:132
        out['mask_rcnn'], out['image'], out['intrinsics'] = mask_rcnn, crop[0], k256[0]
        return out


# ---- the device route ------------------------------------------------------------------------------------------------------
STATUS_BITS = {1: 'a bilinear tap of non-zero weight lies outside the uploaded region of interest',
               2: 'a frame descriptor does not fit the pixel buffer'}


def pack_frames(frames, rois):
    """one uint8 buffer (every sample's block starts 16-byte aligned, the total is a multiple of 16) + the (B,8) int64 descriptors
    {byte offset, row pitch, roi_y0, roi_x0, roi_h, roi_w, frame_H, frame_W} of k_image_crop"""
    desc, blocks, at = [], [], 0
    for frame, (y0, x0, h, w) in zip(frames, rois.tolist()):
        H, W = frame.shape[:2]
        desc.append([at, 3 * w, y0, x0, h, w, H, W])
        block = np.ascontiguousarray(frame[y0:y0 + h, x0:x0 + w]).reshape(-1)
        pad = -block.size % 16
        blocks += [block, np.zeros(pad, np.uint8)] if pad else [block]
        at += block.size + pad
    if at == 0:
        blocks, at = [np.zeros(16, np.uint8)], 16
    return torch.from_numpy(np.concatenate(blocks)), torch.tensor(desc, dtype=torch.int64)


def image_crop(pixels, desc, bboxes, sizes=(SPIN_SIZE, IMAGE_SIZE), normalize=None, status=None):
    """jrr_image_crop on device tensors: pixels uint8 (n,), desc int64 (B,8), bboxes float32 (B,4) -> one (B,3,size,size) float32
    tensor per size from ONE launch; normalize = (mean, std) of 3 values each applies (x - mean) / std to the FIRST size.  `status`
    (int32 (1,), device) collects the kernel's error bits (STATUS_BITS); the caller reads it when it next synchronises."""
    from . import _lib
    lib = _lib.load()
    dev, B = pixels.device, bboxes.shape[0]
    if not 1 <= len(sizes) <= 2:
        raise ValueError('image_crop: one or two crop sizes')
    outs = [torch.empty(B, 3, n, n, device=dev) for n in sizes]
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    mean = std = None
    if normalize is not None:
        mean = torch.tensor(normalize[0], dtype=torch.float32, device=dev)
        std = torch.tensor(normalize[1], dtype=torch.float32, device=dev)
    _lib.check(lib.jrr_image_crop(_lib.ptr(pixels), pixels.numel(), _lib.ptr(desc), _lib.ptr(bboxes), B, _lib.ptr(mean), _lib.ptr(std),
                                  sizes[0], _lib.ptr(outs[0]), sizes[1] if len(sizes) > 1 else 0, _lib.ptr(outs[1]) if len(sizes) > 1 else None,
                                  _lib.ptr(status), _lib.stream_ptr(dev)), 'image_crop')
    return outs


def mask_prepare(masks):
    """jrr_mask_prepare: uint8 (B,h,w) on the device -> (mask_rcnn float32 (B,1,h,w) = mask / 255 with the 2 x 2 corner zeroed,
    valid bool (B,) = mask[:, 0, 0] != 0 before that)  (data.py:121,130-132)"""
    from . import _lib
    lib = _lib.load()
    B, h, w = masks.shape
    out = torch.empty(B, 1, h, w, device=masks.device)
    valid = torch.empty(B, dtype=torch.int32, device=masks.device)
    _lib.check(lib.jrr_mask_prepare(_lib.ptr(masks), B, h, w, _lib.ptr(out), _lib.ptr(valid), _lib.stream_ptr(masks.device)), 'mask_prepare')
    return out, valid != 0


def crop_batch(frames, masks, bboxes, intrinsics, device, sizes=(SPIN_SIZE, IMAGE_SIZE), normalize=None, use_roi: bool = True,
               rois: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The image-valued half of a batch on the device (data.py:110-132 for B samples at once).  frames: B uint8 (H,W,3) arrays (cut to
    [:1000, :1000] here), masks: B uint8 (h,w) arrays of one size, bboxes (B,4), intrinsics (B,3,3) -> device tensors 'spin_image'
    (B,3,sizes[0],sizes[0]), 'image' (B,3,sizes[1],sizes[1]), 'mask_rcnn' (B,1,h,w), 'valid' (B,), 'intrinsics' (B,3,3) of the
    sizes[1] crop, 'min_x', 'min_y', 'scale'.  normalize = (mean, std) normalises 'spin_image' inside the kernel
    (scripts/optimize.py:141-142,164).  use_roi=False uploads whole frames (same result bit for bit); `rois` overrides the blocks.
    Raises _lib.JrrError when the kernel's status word is set."""
    from . import _lib
    frames = [np.asarray(f)[:IMG_RES, :IMG_RES] for f in frames]
    bboxes, intrinsics = torch.as_tensor(bboxes).float().cpu(), torch.as_tensor(intrinsics).float().cpu()
    B = bboxes.shape[0]
    if len(frames) != B or len(masks) != B:
        raise ValueError(f'crop_batch: {len(frames)} frames, {len(masks)} masks, {B} bounding boxes')
    if rois is None:
        rois = torch.stack([crop_roi(bboxes[b:b + 1], *frames[b].shape[:2], sizes=sizes)[0] if use_roi else
                            torch.tensor([0, 0, frames[b].shape[0], frames[b].shape[1]]) for b in range(B)])
    pixels, desc = pack_frames(frames, rois)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    crops = image_crop(pixels.to(device), desc.to(device), bboxes.to(device).contiguous(), sizes, normalize, status)
    mask_rcnn, valid = mask_prepare(torch.from_numpy(np.stack([np.asarray(m) for m in masks])).to(device).contiguous())
    min_x, min_y, scale, k = _crop_geometry(bboxes, intrinsics, sizes[-1])
    bits = int(status.item())                                    # the batch's one synchronisation
    if bits:
        raise _lib.JrrError('image_crop: ' + '; '.join(msg for bit, msg in STATUS_BITS.items() if bits & bit))
    return {'spin_image': crops[0], 'image': crops[-1], 'mask_rcnn': mask_rcnn, 'valid': valid, 'intrinsics': k.to(device),
            'min_x': min_x.to(device), 'min_y': min_y.to(device), 'scale': scale.to(device), 'bytes_uploaded': int(pixels.numel())}
