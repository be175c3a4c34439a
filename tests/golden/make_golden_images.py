#!/usr/bin/env python3
"""Generate tests/golden/g9_find_crop.npz by calling the reference's own scripts.data.find_crop on the CPU.

Run only in the build container (needs /root/reference):  python tests/golden/make_golden_images.py
The reference's Python never travels; only the arrays written here are committed.

scripts/data.py imports h5py and imageio at its top and never uses them in find_crop / crop_intrinsics / resize_intrinsics: empty
stand-in modules take their place.  Inputs come from tests/image_cases.py (seeded), shared with the tests.

Per small case `<name>`: <name>__crop, __min_x, __min_y, __scale, __intrinsics as the reference returns them.  Two scalars:
  ref_f64_err_small   largest |reference fp32 crop - the same formulas in float64| over all small cases
  ref_f64_err_1000    the same over the 37 x 2 large cases at 224 and 256 (no large image is stored)
The float64 evaluation is torch's own grid_sample in double on a grid built in double from the same fp32 bounding boxes: it shares
no code with the package under test.  The tests' bound is 3 x ref_f64_err + 1e-7.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'

sys.argv = ['x', '--device', 'cpu']
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
for name in ('h5py', 'imageio'):
    sys.modules.setdefault(name, types.ModuleType(name))
ref_data = importlib.import_module('scripts.data')
import image_cases as ic  # noqa: E402


def to_image(frame):
    """uint8 (H,W,3) -> float (3,H,W) in [0, 1], cut to 1000 x 1000 (scripts/data.py:111-113)"""
    return torch.from_numpy(frame).permute(2, 0, 1)[:, :1000, :1000].float() / 255.0


def crop_f64(image, bboxes, n):
    """the crop's formulas (scripts/data.py:228-264, sampling_helper.py:46-69, grid_sample bilinear / zeros / align_corners=False) in float64"""
    image, bb = image.double(), bboxes.double()
    if image.dim() == 3:
        image = image[None]
    min_x, max_x, min_y, max_y = ((bb[:, k] - 500) / 500 for k in (1, 3, 0, 2))
    ax, ay = (min_x + max_x) / 2, (min_y + max_y) / 2
    s = torch.maximum(max_x - min_x, max_y - min_y) / 2
    lin = torch.linspace(-1.0, 1.0, n, dtype=torch.float64)
    gx = (s[:, None] * lin[None, :] + (s * (ax / s))[:, None]) / (1 + 1e-8)
    gy = (s[:, None] * lin[None, :] + (s * (ay / s))[:, None]) / (1 + 1e-8)
    grid = torch.stack([gx[:, None, :].expand(-1, n, -1), gy[:, :, None].expand(-1, -1, n)], -1)
    out = torch.nn.functional.grid_sample(image, grid, mode='bilinear', padding_mode='zeros', align_corners=False)
    out[out != out] = 0
    return out


def main():
    arrs = {}
    frames = ic.small_frames()
    err_small = 0.0
    for name, fnames, bboxes, n in ic.SMALL_CASES:
        image = torch.stack([to_image(frames[f]) for f in fnames])
        if len(fnames) == 1:
            image = image[0]                                   # the reference's per-sample call passes (3,H,W)
        bb = torch.tensor(bboxes, dtype=torch.float32)
        k = torch.from_numpy(ic.small_intrinsics(len(fnames)))
        crop, min_x, min_y, scale, k2 = ref_data.find_crop(image, bb.clone(), k.clone(), img_size=n)
        for key, v in (('crop', crop), ('min_x', min_x), ('min_y', min_y), ('scale', scale), ('intrinsics', k2)):
            arrs[f'{name}__{key}'] = v.detach().numpy().astype(np.float32)
        e = (crop.double() - crop_f64(image, bb, n)).abs().max().item()
        print(f'{name:<16s} crop {tuple(crop.shape)}  |fp32 - f64| = {e:.3e}  zeros = {bool((crop == 0).all())}')
        err_small = max(err_small, e)
    err_large = 0.0
    big = ic.large_frames()
    bbs = torch.from_numpy(ic.large_bboxes())
    for fname, frame in big.items():
        image = to_image(frame)
        for i in range(bbs.shape[0]):
            for n in (224, 256):
                crop = ref_data.find_crop(image, bbs[i:i + 1].clone(), torch.eye(3)[None], img_size=n)[0]
                err_large = max(err_large, (crop.double() - crop_f64(image, bbs[i:i + 1], n)).abs().max().item())
    arrs['ref_f64_err_small'] = np.float64(err_small)
    arrs['ref_f64_err_1000'] = np.float64(err_large)
    path = os.path.join(HERE, 'g9_find_crop.npz')
    np.savez_compressed(path, **arrs)
    print(f'ref_f64_err_small = {err_small:.3e}   ref_f64_err_1000 = {err_large:.3e}   {os.path.getsize(path)} bytes')
    assert os.path.getsize(path) <= 400_000


if __name__ == '__main__':
    main()
