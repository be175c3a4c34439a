"""Where the outer batches come from (the reference's scripts/optimize.py:132-139 and scripts/test.py:59-63): the dataset's validation split
(`--data_root`, precomputed tensors in the reference layout, data.py) or seeded synthetic "SPIN-init" batches.
Every batch is a dict of host tensors for the GLOBAL batch -- 'pose6d' (B,24,6), 'betas', 'gt_j3d', 'cam', 'seed', the dataset's also
'gt_j2d' -- which the caller shards; optimize.py and test.py both draw theirs here.
"""
from __future__ import annotations

from typing import Dict, Iterator

import torch

from . import dist as jdist, engine as _engine, smpl_model
from .args import args


def pose_to_rot6d(orient: torch.Tensor, pose: torch.Tensor) -> torch.Tensor:
    """Dataset pose tensors -> (B,24,6) 6-D rotations (x[2i+k] = R[i,k], scripts/utils.py:198-204).
    Accepted: 6-D ((B,1,6)/(B,6) + (B,23,6)/(B,138)), rotation matrices ((B,1,3,3) + (B,23,3,3)) or
    axis-angle ((B,3)/(B,1,3) + (B,69)/(B,23,3); converted by the HIP Rodrigues kernel)."""
    B = pose.shape[0]
    if pose.shape[-1] == 6 or pose.numel() == B * 138:
        return torch.cat([orient.reshape(B, 1, 6), pose.reshape(B, 23, 6)], 1).float().contiguous()
    if pose.numel() == B * 23 * 9:
        R = torch.cat([orient.reshape(B, 1, 3, 3), pose.reshape(B, 23, 3, 3)], 1).float()
    elif pose.numel() == B * 69:
        aa = torch.cat([orient.reshape(B, 1, 3), pose.reshape(B, 23, 3)], 1).float().contiguous()
        R = _engine.rodrigues_forward(aa.reshape(-1, 3)).view(B, 24, 3, 3)
    else:
        raise ValueError(f'unrecognised pose tensor shape {tuple(pose.shape)}')
    return R[..., :, :2].reshape(B, 24, 6).contiguous()


def synthetic_batches(model_np, J_np, B_global: int, n: int, seed: int) -> Iterator[Dict[str, torch.Tensor]]:
    for it in range(n):
        full = smpl_model.synthetic_batch(model_np, J_np, B_global, seed=seed * 1000 + it)
        yield {'pose6d': torch.from_numpy(full['pose6d']), 'betas': torch.from_numpy(full['betas']),
               'gt_j3d': torch.from_numpy(full['gt_j3d']), 'cam': torch.from_numpy(full['cam']), 'seed': seed * 1000 + it}


def _load_agreed(iterator, it: int, device):
    """the loader's next batch, or None with the reason: 1 = it failed to load on some rank (scripts/optimize.py:150-156: reported and
    skipped), 2 = the loader is exhausted.  Under data parallelism every rank loads on its own: the ranks agree on the outcome before
    going on, or a transient error on one rank would pair different batches in the all-reduces that follow (one MAX over a single
    int per batch)."""
    batch, failed = None, 0
    try:
        batch = next(iterator)
    except StopIteration:
        failed = 2
    except Exception as exc:                       # noqa: BLE001  (the reference catches everything here)
        print(f'problem loading batch {it}: {type(exc).__name__}: {exc}')
        failed = 1
    failed = jdist.agree_max(failed, device)
    return (None if failed else batch), failed


class _RefinedRows:
    """`--init_refined`: the samples a refined-pose table (the arrays of refined.load) holds start from ITS pose6d / shape / cam,
    copied exactly; the others keep the dataset's values"""

    def __init__(self, table, n_samples: int):
        if table['has_refined'].shape[0] != n_samples:
            raise ValueError(f'--init_refined: the table holds {table["has_refined"].shape[0]} samples, the dataset {n_samples}')
        self.has = torch.from_numpy(table['has_refined'].astype(bool))
        self.rows = {key: torch.from_numpy(table[name]).float() for key, name in (('pose6d', 'pose6d'), ('betas', 'shape'), ('cam', 'cam'))}

    def substitute(self, out, index):
        idx = index.long()
        has = self.has[idx]
        for key, rows in self.rows.items():
            out[key][has] = rows[idx[has]]


def _image_extras(batch, frames):
    """`--image_masks`: what dataset_images needs to crop a shard of this batch on the device"""
    return dict(index=batch['index'], bboxes=batch['bboxes'].float(), intrinsics=batch['intrinsics'].float(), frames=frames)


def dataset_batches(root: str, B_global: int, seed: int, device, drop_last: bool = False,
                    image_masks: bool = False, with_index: bool = False, init_refined=None) -> Iterator[Dict[str, torch.Tensor]]:
    """scripts/optimize.py:132-137: DataLoader(data_set("validation"), batch_size, shuffle=True, drop_last=False)
    (scripts/test.py:59-63 uses drop_last=True).  image_masks: the samples also carry their index, bounding box and intrinsics, and
    the batch its frame source: the caller crops its shard on the device (dataset_images).  with_index: the batch carries its samples'
    dataset indices and the split's length (`--save_refined`).  init_refined: the arrays of a refined-pose table (`--init_refined`)."""
    from . import data as jdata
    with_index = with_index or init_refined is not None
    frames = jdata.frame_source_for(jdata.split_location('validation', root)) if image_masks else None
    ds = jdata.data_set('validation', root=root, frames=frames, device_crops=image_masks, compute_canada=image_masks and args.compute_canada,
                        with_index=with_index)
    refined_rows = _RefinedRows(init_refined, len(ds)) if init_refined is not None else None
    g = torch.Generator().manual_seed(seed)          # every rank shuffles identically
    loader = torch.utils.data.DataLoader(ds, batch_size=B_global, num_workers=0, shuffle=True, drop_last=drop_last, generator=g)
    iterator = iter(loader)
    for it in range(len(loader)):
        batch, failed = _load_agreed(iterator, it, device)
        if failed == 2:
            return
        if failed:
            continue
        x6 = pose_to_rot6d(batch['orient'].to(device), batch['pose'].to(device)).cpu()
        out = {'pose6d': x6, 'betas': batch['betas'].float(), 'gt_j3d': batch['gt_j3d'].float(), 'cam': batch['cam'].float(),
               'gt_j2d': batch['gt_j2d'].float(), 'seed': seed * 1000 + it}
        if with_index:
            out.update(index=batch['index'], n_samples=len(ds))
        if refined_rows is not None:
            refined_rows.substitute(out, batch['index'])
        if image_masks:
            out.update(_image_extras(batch, frames))
        yield out


def dataset_images(full, lo: int, hi: int, device, size: int) -> Dict[str, torch.Tensor]:
    """scripts/data.py:110-132 for rows [lo, hi) of a dataset batch, on the device: the two crops (the 224 one normalised for the SPIN
    network, scripts/optimize.py:141-142,164), the prepared masks and `valid`.  The loop's rasteriser renders size x size: a mask of
    another size is an error that names the sample."""
    from . import data as jdata
    index = [int(i) for i in full['index'][lo:hi]]
    pairs = [full['frames'].read(i) for i in index]
    for i, (_, mask) in zip(index, pairs):
        if mask.shape != (size, size):
            raise ValueError(f'--image_masks: the mask of sample {i} is {mask.shape[0]} x {mask.shape[1]}, the silhouette term renders {size} x {size}')
    return jdata.crop_batch([p[0] for p in pairs], [p[1] for p in pairs], full['bboxes'][lo:hi], full['intrinsics'][lo:hi], device,
                            normalize=jdata.SPIN_NORMALIZE)
