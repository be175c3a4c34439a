"""Refined poses as per-sample SMPL records (`--save_refined DIR`, `--init_refined DIR`): the pseudo-ground truth the reference's
(dead) /root/reference/scripts/create_smpl_gt.py was meant to produce -- SPIN-style `pose (72) / shape (10)` per frame.

`RefinedTable` owns a zero-initialised (n_rows, 240) device table (the row layout of include/jrr.h, JRR_EXPORT_*) and a status word.
`add()` is ONE launch of k_pose_export per outer batch and shard (csrc/export.hip): the 6-D rotations go through the loop's own
6-D map and the log map, everything else is copied, the rows land at their dataset indices.  Nothing is read back per batch.
`finish()` makes ONE sum-all-reduce under data parallelism (the shards are disjoint and every other rank's rows are zero, so the sum
reproduces every row's values; a stored -0.0 comes back as +0.0 there, since -0.0 + 0.0 = +0.0, so two ranks and one can differ in
the sign bit of a zero -- the only bits `--init_refined` does not get back), then the only read-back, validates, and rank 0 writes `refined.npz` (plain numpy arrays) and `meta.json`.
`finish`, `load` and the validation work on CPU tensors with a gloo group as well.
`RefinedExport` is `--save_refined` as the driver sees it: built once, called where a batch is uploaded, where its joints are scored, after
its J step and at the end of the run.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Optional

import numpy as np
import torch

from . import dist as jdist
from .args import args

LAYOUT_VERSION = 1
ROW = 240                     # include/jrr.h: JRR_EXPORT_ROW and the offsets below
POSE, POSE6D, BETAS, CAM, MARKER, EXTRA, MAX_EXTRA = 0, 72, 216, 226, 229, 230, 10
EXTRA_NAMES = ('joint_err_m', 'joint_err_pa_m', 'joint_sqerr', 'pose_disc_sq', 'shape_disc_sq', 'iou_before', 'iou_after')
STATUS_BITS = {1: 'bit 0: a dataset index lies outside the table (that sample was not stored)',
               2: 'bit 1: a sample was exported twice (its row was overwritten)'}
_TAIL = 4                     # floats behind the table in the flat buffer: one per status bit (summed over the ranks), padding


class RefinedTable:
    def __init__(self, n_rows: int, device):
        self.n_rows = int(n_rows)
        self.flat = torch.zeros(self.n_rows * ROW + _TAIL, device=device)          # what finish() all-reduces and reads back
        self.table = self.flat[:self.n_rows * ROW].view(self.n_rows, ROW)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)

    def add(self, index: torch.Tensor, x6d: torch.Tensor, betas: torch.Tensor, cam: torch.Tensor,
            extras: Optional[Dict[str, Optional[torch.Tensor]]] = None) -> None:
        """one k_pose_export launch: rows `index` (B, int64, on the poses' device: nothing is copied from the host here, a pageable
        upload would wait for the stream) <- the poses' records; `extras` by EXTRA_NAMES, a missing metric is NaN"""
        from . import engine as _engine
        B, dev = x6d.shape[0], x6d.device
        if index.device != dev or index.dtype != torch.int64:
            raise ValueError(f'RefinedTable.add: index must be an int64 tensor on {dev}, got {index.dtype} on {index.device}')
        unknown = set(extras or {}) - set(EXTRA_NAMES)
        if unknown:
            raise ValueError(f'RefinedTable.add: unknown extras {sorted(unknown)}')
        nan = torch.full((B,), float('nan'), device=dev)
        cols = [(extras or {}).get(name) for name in EXTRA_NAMES]
        extra = torch.stack([nan if c is None else c.detach().reshape(B).float() for c in cols], 1).contiguous()
        _engine.pose_export(x6d, betas, cam, index, self.table, self.status, extra=extra)

    def finish(self, directory: str, meta: Optional[dict] = None) -> Dict[str, np.ndarray]:
        """all-reduce, read back, validate; rank 0 writes directory/refined.npz and directory/meta.json.  Returns the arrays."""
        tail = self.flat[self.n_rows * ROW:]
        tail[0:1].copy_((self.status & 1).float())
        tail[1:2].copy_(((self.status >> 1) & 1).float())
        jdist.all_reduce_sum_(self.flat)                                           # THE collective of --save_refined
        host = self.flat.cpu().numpy()                                             # ... and its one read-back
        arrays = unpack(host[:self.n_rows * ROW].reshape(self.n_rows, ROW), status=int(host[-_TAIL] > 0) | (int(host[-_TAIL + 1] > 0) << 1))
        if _rank() == 0:
            os.makedirs(directory, exist_ok=True)
            np.savez(os.path.join(directory, 'refined.npz'), **arrays)
            doc = dict(meta or {}, layout_version=LAYOUT_VERSION, n=self.n_rows, extra_names=list(EXTRA_NAMES),
                       refined=int(arrays['has_refined'].sum()))
            with open(os.path.join(directory, 'meta.json'), 'w') as f:
                json.dump(doc, f, indent=1, sort_keys=True, default=str)
        return arrays


class RefinedExport:
    """`--save_refined DIR` of one run of the driver.  `b` is the driver's batch object (its batch dict `full`, shard bounds, poses and
    per-pose loss terms), `fit` the run's FitReport or None."""

    def __init__(self, directory: str, J_np: np.ndarray, body_model: str):
        import hashlib
        self.directory, self.body_model = directory, body_model
        self.j_hash = hashlib.sha256(np.ascontiguousarray(J_np, dtype=np.float32).tobytes()).hexdigest()[:16]
        self.table = None          # allocated with the first batch: a dataset batch says how many samples the split has

    def upload_index(self, b, device):
        """the shard's rows of the table -- dataset indices, or `it * B_global + row` for synthetic batches: uploaded with the batch,
        ahead of the loop, while the stream is idle"""
        first = b.it * b.B_global
        self.index = (b.full['index'][b.lo:b.hi].to(device, torch.int64) if args.data_root else
                      torch.arange(first + b.lo, first + b.hi, dtype=torch.int64, device=device)).contiguous()

    def evaluate_sums(self, joints: torch.Tensor, gt_mm: torch.Tensor):
        """utils.evaluate_sums -- the same one k_evaluate launch, the sums formed the same way -- with the per-pose output kept"""
        from . import engine as _engine
        with torch.no_grad():
            self.err, self.err_pa = _engine.evaluate(joints.detach().float(), gt_mm.detach().float())
            return self.err.sum(), self.err_pa.sum()

    def add(self, b, fit):
        """one launch, device tensors only; read back once, after the last batch"""
        if self.table is None:
            self.table = RefinedTable(b.full['n_samples'] if args.data_root else args.synthetic_batches * args.batch_size, b.x6d.device)
        self.table.add(self.index, b.x6d, b.betas, b.cam,
                       {'joint_err_m': self.err, 'joint_err_pa_m': self.err_pa, 'joint_sqerr': b.sq, 'pose_disc_sq': b.pose_disc_sq,
                        'shape_disc_sq': b.shape_disc_sq, 'iou_before': fit.iou['before'] if fit is not None else None,
                        'iou_after': fit.iou['after'] if fit is not None else None})

    def finish(self):
        if self.table is None:
            raise RuntimeError('--save_refined: no batch was refined, there is nothing to save')
        flags_doc = {k: v for k, v in vars(args._get()).items() if isinstance(v, (bool, int, float, str, type(None)))}
        self.table.finish(self.directory, {'flags': flags_doc, 'body_model': self.body_model, 'j_regressor_sha256_16': self.j_hash,
                                           'inner_iters': int(args.inner_iters), 'data': 'dataset' if args.data_root else 'synthetic'})


def _rank() -> int:
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank()
    return jdist.env_rank_world()[0]


def unpack(table: np.ndarray, status: int = 0) -> Dict[str, np.ndarray]:
    """(N,240) rows + the status bits -> the arrays of refined.npz; raises on a set status bit or a marker that is not 0 or 1"""
    if table.ndim != 2 or table.shape[1] != ROW:
        raise ValueError(f'refined table: rows of {ROW} floats expected, got {table.shape}')
    if status:
        raise RuntimeError('refined table: status ' + '; '.join(msg for bit, msg in STATUS_BITS.items() if status & bit))
    marker = table[:, MARKER]
    bad = np.nonzero(~((marker == 0) | (marker == 1)))[0]
    if bad.size:
        raise RuntimeError(f'refined table: marker {float(marker[bad[0]])} in row {int(bad[0])} ({bad.size} rows): every sample must be '
                           f'stored by exactly one rank, once')
    table = table.astype(np.float32, copy=False)
    out = {'pose': table[:, POSE:POSE6D].copy(), 'pose6d': table[:, POSE6D:BETAS].reshape(-1, 24, 6).copy(),
           'shape': table[:, BETAS:CAM].copy(), 'cam': table[:, CAM:MARKER].copy(), 'has_refined': (marker == 1).astype(np.uint8)}
    for k, name in enumerate(EXTRA_NAMES):
        out[name] = table[:, EXTRA + k].copy()
    out['mpjpe_mm'] = out['joint_err_m'] * np.float32(1000)
    out['pampjpe_mm'] = out['joint_err_pa_m'] * np.float32(1000)
    return out


def load(directory: str, n: Optional[int] = None) -> Dict[str, np.ndarray]:
    """the arrays of directory/refined.npz (+ 'meta': the dict of meta.json); checks the layout version, the shapes and, when given,
    that the table has `n` rows"""
    with open(os.path.join(directory, 'meta.json')) as f:
        meta = json.load(f)
    if meta.get('layout_version') != LAYOUT_VERSION:
        raise ValueError(f'{directory}: row layout version {meta.get("layout_version")!r}, this build reads version {LAYOUT_VERSION}')
    with np.load(os.path.join(directory, 'refined.npz'), allow_pickle=False) as z:
        out = {k: z[k] for k in z.files}
    N = out['has_refined'].shape[0]
    shapes = {'pose': (N, 72), 'pose6d': (N, 24, 6), 'shape': (N, 10), 'cam': (N, 3), 'has_refined': (N,), 'mpjpe_mm': (N,), 'pampjpe_mm': (N,)}
    shapes.update({name: (N,) for name in EXTRA_NAMES})
    for k, shp in shapes.items():
        if k not in out or out[k].shape != shp:
            raise ValueError(f'{directory}/refined.npz: {k} should be {shp}, is {out[k].shape if k in out else "missing"}')
    if n is not None and N != int(n):
        raise ValueError(f'{directory}: the table holds {N} samples, {int(n)} expected')
    out['meta'] = meta
    return out
