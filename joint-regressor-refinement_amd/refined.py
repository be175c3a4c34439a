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
`smooth()` is `--smooth_refined DIR`: the table along the time axis.  `sequence_runs` orders the refined rows by (camera sequence, frame)
from the frame paths and cuts them into runs of consecutive frames; k_pose_jitter and k_pose_smooth (csrc/smooth.hip) measure and filter
the rotations per run, the existing export writes the filtered records into a copy of the table, and one read-back later
`refined_smooth.npz` holds every array of `refined.npz` plus the jitter before and after.  `refined.npz` is never rewritten.
`fuse_views()` is `--fuse_refined DIR`: the table across the camera views of one instant.  `view_groups` orders the refined rows by
(scene, frame, camera) from the frame paths; k_view_relrot (csrc/views.hip) accumulates each camera's orientation relative to its scene's
reference camera, `relative_rotations` solves the 4x4 eigenproblems on the host, k_view_fuse averages the views of every frame (a
medoid-trimmed quaternion mean per joint, the mean of the shapes), the existing export writes the fused records into a copy of the
table, and `refined_fused.npz` holds every array of its input plus how far each view disagreed with the others.
`place()` is `--place_refined PATH`: the table in the real camera.  The joints of every refined row (`_JointsOf`: the existing SMPL and
find_joints operators under one regressor) against the split's full-frame 2-D joints under its intrinsics: k_place_translation
(csrc/place.hip) solves the three-parameter least-squares problem per pose in fp64, k_place_accumulate fills the table of
place_report.py, and `refined_placed.npz` holds every array of its input plus `trans`, the SMPL transl in the camera frame.
"""
from __future__ import annotations

import json
import os
import re
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import ci_report
from . import eval_protocol
from . import args as jargs
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
        flags_doc = {k: v for k, v in eval_protocol.flags_doc(ci_report.flags_doc(jargs.recorded(args._get()))).items() if isinstance(v, (bool, int, float, str, type(None))) and k not in ('eval_accel', 'regressor_report_depth', 'eval_bones', 'eval_penetration', 'eval_penetration_offset_mm')}
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


def pack(arrays: Dict[str, np.ndarray]) -> np.ndarray:
    """the arrays of refined.npz -> the (N,240) float32 rows they were unpacked from"""
    N = arrays['has_refined'].shape[0]
    table = np.zeros((N, ROW), dtype=np.float32)
    table[:, POSE:POSE6D] = arrays['pose']
    table[:, POSE6D:BETAS] = arrays['pose6d'].reshape(N, BETAS - POSE6D)
    table[:, BETAS:CAM], table[:, CAM:MARKER], table[:, MARKER] = arrays['shape'], arrays['cam'], arrays['has_refined']
    for k, name in enumerate(EXTRA_NAMES):
        table[:, EXTRA + k] = arrays[name]
    return table


def load(directory: str, n: Optional[int] = None, name: str = 'refined.npz') -> Dict[str, np.ndarray]:
    """the arrays of directory/refined.npz -- or of `name`, e.g. SMOOTH_NAME -- (+ 'meta': the dict of meta.json); checks the layout
    version, the shapes and, when given, that the table has `n` rows"""
    with open(os.path.join(directory, 'meta.json')) as f:
        meta = json.load(f)
    if meta.get('layout_version') != LAYOUT_VERSION:
        raise ValueError(f'{directory}: row layout version {meta.get("layout_version")!r}, this build reads version {LAYOUT_VERSION}')
    with np.load(os.path.join(directory, name), allow_pickle=False) as z:
        out = {k: z[k] for k in z.files}
    N = out['has_refined'].shape[0]
    shapes = {'pose': (N, 72), 'pose6d': (N, 24, 6), 'shape': (N, 10), 'cam': (N, 3), 'has_refined': (N,), 'mpjpe_mm': (N,), 'pampjpe_mm': (N,)}
    shapes.update({name: (N,) for name in EXTRA_NAMES})
    for k, shp in shapes.items():
        if k not in out or out[k].shape != shp:
            raise ValueError(f'{directory}/{name}: {k} should be {shp}, is {out[k].shape if k in out else "missing"}')
    if n is not None and N != int(n):
        raise ValueError(f'{directory}: the table holds {N} samples, {int(n)} expected')
    out['meta'] = meta
    return out


def load_path(path: str, n: Optional[int] = None) -> Dict[str, np.ndarray]:
    """`--init_refined PATH`: a directory reads its refined.npz; a path that ends in `.npz` reads that file of its directory"""
    if str(path).endswith('.npz'):
        return load(os.path.dirname(path) or '.', n, name=os.path.basename(path))
    return load(path, n)


# ---- along the time axis (`--smooth_refined`) -------------------------------------------------------------------------------
SMOOTH_NAME = 'refined_smooth.npz'
SMOOTH_MAX_RADIUS = 16        # include/jrr.h: JRR_SMOOTH_MAX_RADIUS
SMOOTH_STATUS_BITS = {1: 'bit 0: an entry of the time order lies outside the table', 2: 'bit 1: a listed row holds no refined pose'}
_FRAME = re.compile(r'^img_(\d+)')


def sequence_key(path) -> Tuple[Optional[str], int]:
    """(sequence key, frame number) of a frame path `.../<action>/imageSequence/<camera>/img_%06d.jpg` (scripts/data.py:301): the key is
    everything up to and including the camera directory, the frame the integer behind `img_`.  (None, -1) for a path without
    `imageSequence`, without a camera directory below it or without a parsable frame number: such a frame is a sequence of its own."""
    parts = re.split(r'[\\/]+', str(path)) if path else []
    if 'imageSequence' not in parts:
        return None, -1
    at = parts.index('imageSequence')
    m = _FRAME.match(parts[-1])
    if at + 2 >= len(parts) or m is None:
        return None, -1
    return '/'.join(parts[:at + 2]), int(m.group(1))


def sequence_runs(paths, has_refined) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(order (M,) int32, run (M,) int32, frame (M,) int64): the table rows with has_refined == 1 in time order -- sorted by (sequence
    key, frame, dataset index) -- and their runs of consecutive frames.  Within a key the stride is the smallest positive frame
    difference between neighbours of that sort; a run is a maximal stretch whose consecutive differences all equal it, so a gap, a
    duplicate frame and an unrefined frame each end the run.  Run ids start at 0 and never decrease.  `paths`: one frame path per row,
    or a pair (keys, frames) of arrays; a row without key (sequence_key; a negative frame in the second form) is a run of length 1
    and sorts behind the keyed rows."""
    has = np.asarray(has_refined).astype(bool)
    N = has.shape[0]
    if isinstance(paths, tuple) and len(paths) == 2 and len(paths[0]) == N and not isinstance(paths[0], str):
        keys, frames = list(np.asarray(paths[0]).tolist()), np.asarray(paths[1]).astype(np.int64)
        keys = [None if f < 0 else k for k, f in zip(keys, frames)]
    else:
        parsed = [sequence_key(p) for p in paths]
        keys, frames = [k for k, _ in parsed], np.array([f for _, f in parsed], dtype=np.int64).reshape(-1)
    if len(keys) != N or frames.shape != (N,):
        raise ValueError(f'sequence_runs: {len(keys)} paths for a table of {N} rows')
    names = sorted({k for k in keys if k is not None})
    lut = {k: i for i, k in enumerate(names)}
    # a row without key gets a key of its own behind every named one, in dataset order
    kid = np.array([lut[k] if k is not None else len(names) + i for i, k in enumerate(keys)], dtype=np.int64).reshape(-1)
    frames = np.where(kid >= len(names), -1, frames)
    idx = np.nonzero(has)[0]
    k, f = kid[idx], frames[idx]
    o = np.lexsort((idx, f, k))
    idx, k, f = idx[o], k[o], f[o]
    if idx.size == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64)
    same, d = k[1:] == k[:-1], f[1:] - f[:-1]
    stride = np.full(len(names) + N, np.iinfo(np.int64).max, dtype=np.int64)
    pos = same & (d > 0)
    np.minimum.at(stride, k[1:][pos], d[pos])
    cont = pos & (d == stride[k[1:]])
    run = np.concatenate([[0], np.cumsum(~cont)])
    return idx.astype(np.int32), run.astype(np.int32), f.astype(np.int64)


def smooth_weights(sigma: float, radius: Optional[int] = None) -> np.ndarray:
    """weights[k] = float32(exp(-k^2 / (2 sigma^2))), k = 0 .. radius, evaluated in float64 and rounded once; radius None:
    min(16, ceil(3 sigma))"""
    sigma = float(sigma)
    if not (sigma > 0 and np.isfinite(sigma)):
        raise ValueError(f'smooth: sigma {sigma}: a positive number')
    radius = min(SMOOTH_MAX_RADIUS, int(np.ceil(3 * sigma))) if radius is None else int(radius)
    if not 0 <= radius <= SMOOTH_MAX_RADIUS:
        raise ValueError(f'smooth: radius {radius}: 0 .. {SMOOTH_MAX_RADIUS}')
    k = np.arange(radius + 1, dtype=np.float64)
    return np.exp(-(k * k) / (2.0 * sigma * sigma)).astype(np.float32)


def _nanmean(x) -> Optional[float]:
    x = np.asarray(x, dtype=np.float64)
    x = x[~np.isnan(x)]
    return float(x.mean()) if x.size else None


def smooth(directory: str, paths, sigma: float = 2.0, radius: Optional[int] = None, device=None, rescore=None) -> Dict[str, np.ndarray]:
    """`--smooth_refined DIR`: the table of DIR/refined.npz filtered along time.  Uploads the table, measures its jitter
    (jrr_pose_jitter), filters it (jrr_pose_smooth), writes the filtered records into a COPY of the table with the existing pose_export
    operator -- so the smoothed `pose` is the same log map of the same 6-D map as in refined.npz --, measures the copy's jitter and
    reads everything back once.  Writes DIR/refined_smooth.npz (every array of refined.npz + jitter_deg_raw / jitter_deg /
    smooth_delta_deg, NaN outside the time order, and run_id / run_len / frame, -1 there) and adds `smooth` to DIR/meta.json;
    refined.npz is not rewritten.  `paths` as sequence_runs takes them.  `rescore(raw, smoothed) -> (arrays, numbers)`: more
    per-sample arrays for the file and numbers for meta.json, computed before the one write.  Returns the arrays."""
    from . import engine as _engine
    raw = load(directory)
    meta = raw.pop('meta')
    N = raw['has_refined'].shape[0]
    order, run, frame = sequence_runs(paths, raw['has_refined'])
    weights = smooth_weights(sigma, radius)
    M, rad = order.shape[0], weights.shape[0] - 1
    device = torch.device(args.device if device is None else device)
    host_table = pack(raw)
    if M:
        table = torch.from_numpy(host_table).to(device)
        d_order, d_run, d_w = (torch.from_numpy(a).to(device) for a in (order, run, weights))
        status, status_x = torch.zeros(1, dtype=torch.int32, device=device), torch.zeros(1, dtype=torch.int32, device=device)
        jit_raw = _engine.pose_jitter(table, d_order, d_run, status)
        x6d, betas, cam, delta = _engine.pose_smooth(table, d_order, d_run, d_w, status)
        rows = d_order.long()
        copy = table.clone()
        copy[rows, MARKER] = 0                                     # the export claims the rows it writes
        _engine.pose_export(x6d, betas, cam, rows, copy, status_x, extra=table[rows, EXTRA:EXTRA + len(EXTRA_NAMES)].contiguous())
        jit = _engine.pose_jitter(copy, d_order, d_run, status)
        flat = torch.cat([copy.reshape(-1), jit_raw, jit, delta, status.float(), status_x.float()]).cpu().numpy()     # the one read-back
        st, st_x = int(flat[-2]), int(flat[-1])
        if st:
            raise RuntimeError('smooth: status ' + '; '.join(msg for bit, msg in SMOOTH_STATUS_BITS.items() if st & bit))
        host_table = flat[:N * ROW].reshape(N, ROW)
        per_pos = flat[N * ROW:N * ROW + 3 * M].reshape(3, M)
    else:
        st_x, per_pos = 0, np.zeros((3, 0), dtype=np.float32)
    out = unpack(host_table, status=st_x)
    for k, name in enumerate(('jitter_deg_raw', 'jitter_deg', 'smooth_delta_deg')):
        out[name] = np.full(N, np.nan, dtype=np.float32)
        out[name][order] = per_pos[k]
    n_runs = int(run[-1]) + 1 if M else 0
    lengths = np.bincount(run, minlength=n_runs)
    out['run_id'], out['run_len'], out['frame'] = np.full(N, -1, np.int32), np.full(N, -1, np.int32), np.full(N, -1, np.int64)
    out['run_id'][order], out['run_len'][order], out['frame'][order] = run, lengths[run], frame
    hist = np.bincount(lengths) if M else np.zeros(0, dtype=np.int64)
    doc = {'sigma': float(sigma), 'radius': int(rad), 'positions': int(M), 'runs': n_runs,
           'run_length_histogram': {str(n): int(c) for n, c in enumerate(hist) if c},
           'jitter_deg_raw_mean': _nanmean(out['jitter_deg_raw']), 'jitter_deg_mean': _nanmean(out['jitter_deg']),
           'smooth_delta_deg_mean': _nanmean(out['smooth_delta_deg'])}
    if rescore is not None:
        more, numbers = rescore(raw, out)
        out.update(more)
        doc.update(numbers)
    np.savez(os.path.join(directory, SMOOTH_NAME), **out)
    with open(os.path.join(directory, 'meta.json'), 'w') as f:
        json.dump(dict(meta, smooth=doc), f, indent=1, sort_keys=True, default=str)
    out['meta'] = dict(meta, smooth=doc)
    return out


class _JointsOf:
    """the 17 joints of table rows through the EXISTING operators: SMPL as the driver resolves it and RefineEngine.find_joints_forward
    under ONE regressor (--eval_j_regressor, else the initial one) with the mask of the initial one.  Called with a table's arrays and
    a chunk of row numbers; returns the (len(rows),17,3) device tensor, not pelvis-centred.  One engine per chunk size."""

    def __init__(self, device):
        from . import checkpoint, smpl_model, utils
        from .smpl import SMPL
        self.device = device
        self.smpl = SMPL(args.smpl_dir, batch_size=1, allow_synthetic=args.synthetic or args.smpl_dir == 'SPIN/data/smpl').to(device)
        J_np = smpl_model.default_h36m_regressor(args.j_regressor_init,
                                                 allow_default=args.synthetic or args.j_regressor_init == 'SPIN/data/J_regressor_h36m.npy')
        J_init = torch.from_numpy(J_np).float().to(device)
        self.J = checkpoint.load_j_regressor(args.eval_j_regressor).float().to(device) if args.eval_j_regressor else J_init
        self.mask = utils.find_j_reg_mask(J_init)
        self.name = args.eval_j_regressor or args.j_regressor_init
        self.engines: Dict[int, object] = {}

    def __call__(self, arrays, rows) -> torch.Tensor:
        from . import engine as _engine
        B = int(len(rows))
        if B not in self.engines:
            self.engines[B] = _engine.RefineEngine(self.smpl.device_model, B)
            self.engines[B].set_j_regressor(self.J, self.mask)
        x6d = torch.from_numpy(arrays['pose6d'][rows]).to(self.device).float().contiguous()
        betas = torch.from_numpy(arrays['shape'][rows]).to(self.device).float().contiguous()
        return self.engines[B].find_joints_forward(betas, x6d=x6d)


def _rescore_fn(gt_j3d_mm: torch.Tensor, device, tag: str = 'smooth', accel_paths=None):
    """the joint error of the raw and the smoothed (`tag`: the suffix of the second pair of names) rows through the EXISTING operators -- SMPL, find_joints, jrr_evaluate_joints -- in
    chunks of --batch_size under ONE regressor (--eval_j_regressor, else the initial one), the body as the driver resolves it.
    `accel_paths` (the split's frame paths, under --eval_accel): the joints of both passes are kept in device tables at their
    dataset indices, and jrr_accel_error gives accel_err_mm_raw / accel_err_mm_<tag> along the runs of the table's refined rows."""
    from . import engine as _engine, utils

    def rescore(raw, smoothed):
        joints_of = _JointsOf(device)
        rows = np.nonzero(raw['has_refined'])[0]
        N, bs = raw['has_refined'].shape[0], max(1, int(args.batch_size))
        acc = torch.full((4, N), float('nan'), device=device)
        kept = torch.zeros((3, N, 17, 3), device=device) if accel_paths is not None else None        # raw | processed | ground truth
        with torch.no_grad():
            for a in range(0, rows.size, bs):
                idx = torch.from_numpy(rows[a:a + bs])
                gt = utils.move_pelvis(gt_j3d_mm[idx].to(device).float())
                d_idx = idx.to(device)
                if kept is not None:
                    kept[2, d_idx] = gt
                for k, arrays in enumerate((raw, smoothed)):
                    joints = joints_of(arrays, rows[a:a + bs])
                    err_j, err_pa_j = _engine.evaluate_joints(joints.float().contiguous(), gt.contiguous())
                    acc[2 * k, d_idx] = err_j.mean(1) * 1000
                    acc[2 * k + 1, d_idx] = err_pa_j.mean(1) * 1000
                    if kept is not None:
                        kept[k, d_idx] = joints.float()
        host = acc.cpu().numpy()
        names = ('mpjpe_eval_mm_raw', 'pampjpe_eval_mm_raw', 'mpjpe_eval_mm_' + tag, 'pampjpe_eval_mm_' + tag)
        more = {name: host[k] for k, name in enumerate(names)}
        numbers = {name + '_mean': _nanmean(host[k]) for k, name in enumerate(names)}
        if kept is not None:
            from . import accel_report
            for name, values in zip(('accel_err_mm_raw', 'accel_err_mm_' + tag),
                                    accel_report.per_sample_mm((kept[0], kept[1]), kept[2], accel_paths, raw['has_refined'])):
                more[name], numbers[name + '_mean'] = values, _nanmean(values)
        numbers['eval_j_regressor'] = args.eval_j_regressor or args.j_regressor_init
        return more, numbers
    return rescore


def smooth_command(log=print) -> Optional[dict]:
    """`python main.py --smooth_refined DIR --data_root ROOT [--smooth_sigma S] [--smooth_radius R]`: refined.smooth on the split the
    table was written from, the frame paths from its images.pkl, plus the joint error of the raw and the smoothed rows.  One process:
    under torchrun rank 0 works and the other ranks return.  Prints one summary line."""
    from . import data as jdata
    if jdist.env_rank_world()[0] != 0:                      # the command joins no process group: the launcher's rank decides
        return None
    if not args.data_root:
        raise ValueError('--smooth_refined needs --data_root (the frame paths and the ground truth of the split the table was written from)')
    location = jdata.split_location('validation', args.data_root)
    paths = jdata.split_image_paths(location)
    if paths is None:
        raise FileNotFoundError(f'--smooth_refined: {os.path.join(location, "images.pkl")} is missing: the frame paths say which samples follow each other')
    ds = jdata.data_set('validation', root=args.data_root)
    n_table = load(args.smooth_refined)['has_refined'].shape[0]
    if not (len(paths) == len(ds) == n_table):
        raise ValueError(f'--smooth_refined: the table holds {n_table} samples, the split {len(ds)} with {len(paths)} frame paths')
    device = torch.device(args.device)
    torch.cuda.set_device(device)
    out = smooth(args.smooth_refined, paths, sigma=args.smooth_sigma, radius=args.smooth_radius, device=device,
                 rescore=_rescore_fn(ds.gt_j3d, device, accel_paths=paths if args.eval_accel else None))
    doc = out['meta']['smooth']
    fmt = lambda v, spec='.4f': '-' if v is None else format(v, spec)
    accel = f', accel error {fmt(doc["accel_err_mm_raw_mean"])} -> {fmt(doc["accel_err_mm_smooth_mean"])} mm/frame^2' if args.eval_accel else ''
    log(f'smoothed {doc["positions"]} poses in {doc["runs"]} runs (sigma {doc["sigma"]:g}, radius {doc["radius"]}): jitter '
        f'{fmt(doc["jitter_deg_raw_mean"])} -> {fmt(doc["jitter_deg_mean"])} deg/frame^2, moved {fmt(doc["smooth_delta_deg_mean"])} deg, MPJPE '
        f'{fmt(doc["mpjpe_eval_mm_raw_mean"])} -> {fmt(doc["mpjpe_eval_mm_smooth_mean"])}, PAMPJPE {fmt(doc["pampjpe_eval_mm_raw_mean"])} -> '
        f'{fmt(doc["pampjpe_eval_mm_smooth_mean"])}{accel}; {os.path.join(args.smooth_refined, SMOOTH_NAME)}')
    return out


# ---- across the camera views of one instant (`--fuse_refined`) --------------------------------------------------------------
FUSE_NAME = 'refined_fused.npz'
FUSE_MAX_VIEWS = 8            # include/jrr.h: JRR_FUSE_MAX_VIEWS
FUSE_ACC_ROW = 12             # include/jrr.h: JRR_FUSE_ACC_ROW
FUSE_STATUS_BITS = {1: 'bit 0: an entry of the view order lies outside the table', 2: 'bit 1: a listed row holds no refined pose',
                    4: 'bit 2: a group continues beyond the 7 positions on either side', 8: 'bit 3: a pair id outside [0, n_pairs)'}


def view_key(path) -> Tuple[Optional[str], Optional[str], int]:
    """(scene, camera, frame) of a frame path `<scene>/imageSequence/<camera>/img_%06d.jpg`: the scene is everything before
    `imageSequence`, the camera the directory below it, the frame as sequence_key reads it.  (None, None, -1) for a path sequence_key
    refuses."""
    key, frame = sequence_key(path)
    if key is None:
        return None, None, -1
    parts = key.split('/')
    return '/'.join(parts[:-2]), parts[-1], frame


def view_groups(paths, has_refined):
    """(order (M,) int32, group (M,) int32, pair (M,) int32, ref_pair (n_pairs,) int32, names, duplicates): the table rows with
    has_refined == 1 ordered by (scene, frame, camera, dataset index) and cut into groups -- one per (scene, frame), its members
    contiguous and in camera order; group ids start at 0 and never decrease.  A second row with the (scene, frame, camera) of an earlier
    one is a DUPLICATE: a group of one directly behind the group of its frame, counted in `duplicates`.  A row without key (view_key)
    is a group of one behind all keyed rows, in dataset order.  pair: the id of the position's (scene, camera) in [0, n_pairs) -- the
    pairs that occur, sorted by (scene, camera); `names[c]` is that (scene, camera) -- or -1 for keyless rows and duplicates.
    ref_pair[c]: the pair of the scene's reference camera, its first camera in sorted order (ref_pair[c] == c for that camera).
    A group of more than 8 members raises ValueError.  `paths`: one frame path per row, or arrays (scenes, cameras, frames) -- or
    (cameras, frames) for a single scene -- where a negative frame marks a row without key."""
    has = np.asarray(has_refined).astype(bool)
    N = has.shape[0]
    if isinstance(paths, tuple) and len(paths) in (2, 3) and not isinstance(paths[0], str) and len(paths[0]) == N:
        cols = [np.asarray(a).tolist() for a in paths]
        scenes, cams, frames = ([0] * N, cols[0], cols[1]) if len(paths) == 2 else cols
        parsed = [(None, None, -1) if f < 0 else (sc, c, int(f)) for sc, c, f in zip(scenes, cams, frames)]
    else:
        parsed = [view_key(p) for p in paths]
    if len(parsed) != N:
        raise ValueError(f'view_groups: {len(parsed)} paths for a table of {N} rows')
    idx = np.nonzero(has)[0]
    keyed = [int(i) for i in idx if parsed[i][0] is not None]
    stray = [int(i) for i in idx if parsed[i][0] is None]
    keyed.sort(key=lambda i: (parsed[i][0], parsed[i][2], parsed[i][1], i))
    dup = [k > 0 and parsed[keyed[k]] == parsed[keyed[k - 1]] for k in range(len(keyed))]
    names = sorted({(parsed[i][0], parsed[i][1]) for i in keyed})
    lut = {n: c for c, n in enumerate(names)}
    first = {}
    for c, (scene, _) in enumerate(names):
        first.setdefault(scene, c)
    ref_pair = np.array([first[scene] for scene, _ in names], dtype=np.int32).reshape(-1)
    order, group, pair = [], [], []
    g, at = -1, 0
    while at < len(keyed):
        end = at
        while end < len(keyed) and parsed[keyed[end]][0] == parsed[keyed[at]][0] and parsed[keyed[end]][2] == parsed[keyed[at]][2]:
            end += 1
        members = [k for k in range(at, end) if not dup[k]]
        if len(members) > FUSE_MAX_VIEWS:
            raise ValueError(f'view_groups: {len(members)} views of frame {parsed[keyed[at]][2]} of {parsed[keyed[at]][0]!r}: at most {FUSE_MAX_VIEWS}')
        g += 1
        for k in members:
            order.append(keyed[k]); group.append(g); pair.append(lut[parsed[keyed[k]][:2]])
        for k in range(at, end):
            if dup[k]:
                g += 1
                order.append(keyed[k]); group.append(g); pair.append(-1)
        at = end
    for i in stray:
        g += 1
        order.append(i); group.append(g); pair.append(-1)
    as32 = lambda a: np.array(a, dtype=np.int32).reshape(-1)
    return as32(order), as32(group), as32(pair), ref_pair, names, int(sum(dup))


def relative_rotations(acc, ref_pair=None) -> Tuple[np.ndarray, np.ndarray]:
    """(rel (n_pairs, 4) float32, residual_deg (n_pairs,) float64) of the table jrr_view_relrot_accumulate filled: per pair the 4x4
    symmetric matrix acc / (2^24 count) in float64, the eigenvector of its largest eigenvalue lambda (numpy.linalg.eigh) with w >= 0 --
    the rotation d_c with R_ref ~ D_c R_c -- and 2 acos(sqrt(min(1, lambda))) in degrees, the RMS-like spread of the per-frame relative
    rotations about d_c.  A reference camera (ref_pair[c] == c) gets (1, 0, 0, 0) and residual 0; a pair with count 0 gets (0, 0, 0, 0),
    meaning unknown, and residual NaN."""
    acc = np.asarray(acc, dtype=np.int64).reshape(-1, FUSE_ACC_ROW)
    n = acc.shape[0]
    rel, res = np.zeros((n, 4), dtype=np.float64), np.full(n, np.nan)
    iu = np.triu_indices(4)
    for c in range(n):
        if ref_pair is not None and int(ref_pair[c]) == c:
            rel[c], res[c] = (1.0, 0.0, 0.0, 0.0), 0.0
            continue
        if acc[c, 0] <= 0:
            continue
        A = np.zeros((4, 4))
        A[iu] = acc[c, 1:11].astype(np.float64) / (2.0 ** 24 * float(acc[c, 0]))
        A = A + np.triu(A, 1).T
        lam, U = np.linalg.eigh(A)
        d = U[:, -1]
        rel[c] = -d if d[0] < 0 else d
        res[c] = np.degrees(2.0 * np.arccos(np.sqrt(min(1.0, max(0.0, float(lam[-1]))))))
    return rel.astype(np.float32), res


def _axis_angle_deg(q) -> list:
    q = np.asarray(q, dtype=np.float64)
    n = float(np.linalg.norm(q[1:]))
    if n == 0.0:
        return [0.0, 0.0, 0.0]
    return (q[1:] / n * np.degrees(2.0 * np.arctan2(n, abs(q[0]))) * (1.0 if q[0] >= 0 else -1.0)).tolist()


def fuse_views(directory_or_npz: str, paths, max_deg: float = 30.0, device=None, rescore=None) -> Dict[str, np.ndarray]:
    """`--fuse_refined DIR`: the table of DIR/refined.npz -- or of the named `.npz` of its directory, as load_path reads it -- fused across
    the camera views of each (scene, frame).  Uploads the table, accumulates every camera's orientation relative to its scene's reference
    camera (jrr_view_relrot_accumulate), reads that small table back and solves it (relative_rotations), fuses the views
    (jrr_view_fuse; max_deg 0 selects the plain mean) and writes the fused records -- with each row's OWN cam and extras -- into a COPY of
    the table with the existing pose_export operator, so the fused `pose` is the same log map of the same 6-D map; one more read-back.
    Writes DIR/refined_fused.npz (every array of the input + view_group / n_views / view_pair, -1 outside the order, fuse_delta_body_deg /
    fuse_delta_orient_deg, NaN there, and fuse_dropped) and adds `fuse` to DIR/meta.json; the input file is not rewritten.  `paths` as
    view_groups takes them, `rescore` as in smooth().  Returns the arrays."""
    from . import engine as _engine
    max_deg = float(max_deg)
    if not (0.0 <= max_deg <= 360.0):
        raise ValueError(f'fuse_views: max_deg {max_deg}: 0 (the plain mean) .. 360')
    directory = (os.path.dirname(directory_or_npz) or '.') if str(directory_or_npz).endswith('.npz') else directory_or_npz
    raw = load_path(directory_or_npz)
    meta = raw.pop('meta')
    N = raw['has_refined'].shape[0]
    order, group, pair, ref_pair, names, duplicates = view_groups(paths, raw['has_refined'])
    M, n_pairs = order.shape[0], ref_pair.shape[0]
    cos_half_max = float(np.float32(np.cos(np.radians(max_deg) / 2.0))) if max_deg > 0 else 0.0
    device = torch.device(args.device if device is None else device)
    host_table = pack(raw)
    acc = np.zeros((n_pairs, FUSE_ACC_ROW), dtype=np.int64)
    if M:
        table = torch.from_numpy(host_table).to(device)
        d_order, d_group, d_pair, d_ref = (torch.from_numpy(a).to(device) for a in (order, group, pair, ref_pair))
        status, status_x = torch.zeros(1, dtype=torch.int32, device=device), torch.zeros(1, dtype=torch.int32, device=device)
        d_acc = torch.zeros((n_pairs, FUSE_ACC_ROW), dtype=torch.int64, device=device)
        _engine.view_relrot_accumulate(table, d_order, d_group, d_pair, d_ref, d_acc, status)
        acc = d_acc.cpu().numpy()                                  # the 4x4 solves need it
    rel, residual = relative_rotations(acc, ref_pair)
    if M:
        x6d, betas, d_body, d_orient, members, dropped = _engine.view_fuse(table, d_order, d_group, d_pair, torch.from_numpy(rel).to(device),
                                                                           cos_half_max, status)
        rows = d_order.long()
        copy = table.clone()
        copy[rows, MARKER] = 0                                     # the export claims the rows it writes
        _engine.pose_export(x6d, betas, table[rows, CAM:MARKER].contiguous(), rows, copy, status_x,
                            extra=table[rows, EXTRA:EXTRA + len(EXTRA_NAMES)].contiguous())
        flat = torch.cat([copy.reshape(-1), d_body, d_orient, members.float(), dropped.float(), status.float(), status_x.float()]).cpu().numpy()
        st, st_x = int(flat[-2]), int(flat[-1])                    # ... the one read-back behind the last launch
        if st:
            raise RuntimeError('fuse_views: status ' + '; '.join(msg for bit, msg in FUSE_STATUS_BITS.items() if st & bit))
        host_table = flat[:N * ROW].reshape(N, ROW)
        per_pos = flat[N * ROW:N * ROW + 4 * M].reshape(4, M)
    else:
        st_x, per_pos = 0, np.zeros((4, 0), dtype=np.float32)
    out = dict(raw)
    out.update(unpack(host_table, status=st_x))
    for k, name in enumerate(('fuse_delta_body_deg', 'fuse_delta_orient_deg')):
        out[name] = np.full(N, np.nan, dtype=np.float32)
        out[name][order] = per_pos[k]
    out['view_group'], out['n_views'], out['view_pair'] = (np.full(N, -1, np.int32) for _ in range(3))
    out['view_group'][order], out['n_views'][order], out['view_pair'][order] = group, per_pos[2].astype(np.int32), pair
    out['fuse_dropped'] = np.zeros(N, np.int32)
    out['fuse_dropped'][order] = per_pos[3].astype(np.int32)
    n_groups = int(group[-1]) + 1 if M else 0
    hist = np.bincount(np.bincount(group, minlength=n_groups)) if M else np.zeros(0, dtype=np.int64)
    doc = {'max_deg': max_deg, 'positions': int(M), 'groups': n_groups, 'duplicates': int(duplicates),
           'views_per_group_histogram': {str(n): int(c) for n, c in enumerate(hist) if c},
           'pairs': [{'scene': str(scene), 'camera': str(camera), 'count': int(acc[c, 0]), 'reference': bool(ref_pair[c] == c),
                      'd_axis_angle_deg': _axis_angle_deg(rel[c]), 'residual_deg': None if np.isnan(residual[c]) else float(residual[c])}
                     for c, (scene, camera) in enumerate(names)],
           'fuse_delta_body_deg_mean': _nanmean(out['fuse_delta_body_deg']), 'fuse_delta_orient_deg_mean': _nanmean(out['fuse_delta_orient_deg']),
           'dropped_share': float(out['fuse_dropped'].sum()) / (24.0 * M) if M else None}
    if rescore is not None:
        more, numbers = rescore(raw, out)
        out.update(more)
        doc.update(numbers)
    np.savez(os.path.join(directory, FUSE_NAME), **out)
    with open(os.path.join(directory, 'meta.json'), 'w') as f:
        json.dump(dict(meta, fuse=doc), f, indent=1, sort_keys=True, default=str)
    out['meta'] = dict(meta, fuse=doc)
    return out


def fuse_command(log=print) -> Optional[dict]:
    """`python main.py --fuse_refined DIR --data_root ROOT [--fuse_max_deg 30]`: refined.fuse_views on the split the table was written
    from, the frame paths from its images.pkl, plus the joint error of the raw and the fused rows -- each row in its own camera's frame,
    the frame of its gt_j3d.  One process: under torchrun rank 0 works and the other ranks return.  Prints one summary line."""
    from . import data as jdata
    if jdist.env_rank_world()[0] != 0:                      # the command joins no process group: the launcher's rank decides
        return None
    if not args.data_root:
        raise ValueError('--fuse_refined needs --data_root (the frame paths and the ground truth of the split the table was written from)')
    location = jdata.split_location('validation', args.data_root)
    paths = jdata.split_image_paths(location)
    if paths is None:
        raise FileNotFoundError(f'--fuse_refined: {os.path.join(location, "images.pkl")} is missing: the frame paths say which samples show the same instant')
    ds = jdata.data_set('validation', root=args.data_root)
    n_table = load_path(args.fuse_refined)['has_refined'].shape[0]
    if not (len(paths) == len(ds) == n_table):
        raise ValueError(f'--fuse_refined: the table holds {n_table} samples, the split {len(ds)} with {len(paths)} frame paths')
    device = torch.device(args.device)
    torch.cuda.set_device(device)
    out = fuse_views(args.fuse_refined, paths, max_deg=args.fuse_max_deg, device=device, rescore=_rescore_fn(ds.gt_j3d, device, tag='fused', accel_paths=paths if args.eval_accel else None))
    doc = out['meta']['fuse']
    fmt = lambda v, spec='.4f': '-' if v is None else format(v, spec)
    accel = f', accel error {fmt(doc["accel_err_mm_raw_mean"])} -> {fmt(doc["accel_err_mm_fused_mean"])} mm/frame^2' if args.eval_accel else ''
    directory = (os.path.dirname(args.fuse_refined) or '.') if str(args.fuse_refined).endswith('.npz') else args.fuse_refined
    log(f'fused {doc["positions"]} poses in {doc["groups"]} groups over {len(doc["pairs"])} cameras (max {doc["max_deg"]:g} deg, '
        f'{doc["duplicates"]} duplicates): body moved {fmt(doc["fuse_delta_body_deg_mean"])} deg, orientation '
        f'{fmt(doc["fuse_delta_orient_deg_mean"])} deg, dropped {fmt(doc["dropped_share"])}, MPJPE {fmt(doc["mpjpe_eval_mm_raw_mean"])} -> '
        f'{fmt(doc["mpjpe_eval_mm_fused_mean"])}, PAMPJPE {fmt(doc["pampjpe_eval_mm_raw_mean"])} -> {fmt(doc["pampjpe_eval_mm_fused_mean"])}{accel}; '
        f'{os.path.join(directory, FUSE_NAME)}')
    return out


# ---- in the real camera (`--place_refined`) -----------------------------------------------------------------------------------
PLACE_NAME = 'refined_placed.npz'
PLACE_MAX_ITERS = 64          # include/jrr.h: JRR_PLACE_MAX_ITERS


def place(directory_or_npz: str, intrinsics, gt_j2d, paths, joints_of, n_iters: int = 10, weights=None, weights_name: Optional[str] = None,
          batch_size: int = 256, group_kind: str = 'action', gt_j3d_mm=None, device=None) -> Dict[str, np.ndarray]:
    """`--place_refined PATH`: the camera-frame translation of every refined row of DIR/refined.npz -- or of the named `.npz` of its
    directory, as load_path reads it -- under the split's real intrinsics (N,3,3) and FULL-FRAME 2-D joints gt_j2d (N,17,2).
    `joints_of(arrays, rows)` gives the (len(rows),17,3) joints of table rows on the device (_JointsOf).  Per chunk of `batch_size`
    rows: jrr_place_translation twice (0 steps: the linear start; n_iters steps: the result) and jrr_place_accumulate into the table of
    place_report by the groups of `paths` (None: one group); then the table and everything per pose are read back once each.  Writes
    DIR/refined_placed.npz -- every array of the input unchanged + trans / trans_linear (N,3) float64 m, reproj_px / reproj_px_linear
    (N,17) float32, NaN on rows without a refined pose, and place_status (N,) int32, -1 there --, DIR/place.json, DIR/place.md and the
    entry `place` of DIR/meta.json; the input file is not rewritten.  weights (N,17) or None: ones.  gt_j3d_mm (N,17,3): when some row's
    pelvis lies further than 1 mm from the origin the ground truth is in the camera frame, and the distance of the placed pelvis from
    the measured one is reported as root_err_mm; otherwise the key is absent.  Returns the arrays."""
    from . import engine as _engine, eval_report, place_report
    n_iters = int(n_iters)
    if not 0 <= n_iters <= PLACE_MAX_ITERS:
        raise ValueError(f'place: n_iters {n_iters}: 0 .. {PLACE_MAX_ITERS}')
    directory = (os.path.dirname(directory_or_npz) or '.') if str(directory_or_npz).endswith('.npz') else directory_or_npz
    raw = load_path(directory_or_npz)
    meta = raw.pop('meta')
    N = raw['has_refined'].shape[0]
    as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    intrinsics, gt_j2d = as_t(intrinsics).float(), as_t(gt_j2d).float()
    for name, t, shape in (('intrinsics', intrinsics, (N, 3, 3)), ('gt_j2d', gt_j2d, (N, 17, 2))) + \
            ((('weights', as_t(weights), (N, 17)),) if weights is not None else ()) + \
            ((('gt_j3d', as_t(gt_j3d_mm), (N, 17, 3)),) if gt_j3d_mm is not None else ()):
        if tuple(t.shape) != shape:
            raise ValueError(f'place: {name} should be {shape} for a table of {N} samples, is {tuple(t.shape)}')
    weights = None if weights is None else as_t(weights).float()
    names, gid = eval_report.assign_groups(paths, group_kind, n=N)
    if gid.shape[0] != N:
        raise ValueError(f'place: {gid.shape[0]} paths for a table of {N} rows')
    G = len(names)
    device = torch.device(args.device if device is None else device)
    rows = np.nonzero(raw['has_refined'])[0]
    M, bs = int(rows.size), max(1, int(batch_size))
    root_err = gt_j3d_mm is not None and bool((as_t(gt_j3d_mm).float()[:, 0].norm(dim=1) > 1.0).any())
    trans, trans_lin = (torch.full((M, 3), float('nan'), dtype=torch.float64, device=device) for _ in range(2))
    err, err_lin = (torch.full((M, 17), float('nan'), device=device) for _ in range(2))
    status, status_lin = (torch.full((M,), -1, dtype=torch.int32, device=device) for _ in range(2))
    root = torch.full((M,), float('nan'), dtype=torch.float64, device=device)
    acc = torch.zeros(G * place_report.ROW + place_report.TRAILER, dtype=torch.int64, device=device)
    with torch.no_grad():
        for a in range(0, M, bs):
            idx = torch.from_numpy(rows[a:a + bs])
            s = slice(a, a + int(idx.shape[0]))
            joints = joints_of(raw, rows[a:a + bs]).float().contiguous()
            K, j2d = intrinsics[idx].to(device).contiguous(), gt_j2d[idx].to(device).contiguous()
            w = None if weights is None else weights[idx].to(device).contiguous()
            _engine.place_translation(joints, j2d, K, w, 0, out=(trans_lin[s], None, err_lin[s], status_lin[s]))
            _engine.place_translation(joints, j2d, K, w, n_iters, out=(trans[s], None, err[s], status[s]))
            _engine.place_accumulate(trans[s], err_lin[s], err[s], w, status[s], torch.from_numpy(gid[rows[a:a + bs]]).to(device), G, acc)
            if root_err:
                root[s] = (trans[s] + joints[:, 0].double() - as_t(gt_j3d_mm)[idx][:, 0].to(device).double() / 1000).norm(dim=1) * 1000
    table = place_report.derive(acc.cpu().numpy(), names)                     # the table ...
    flat = torch.cat([trans.reshape(-1), trans_lin.reshape(-1), err.double().reshape(-1), err_lin.double().reshape(-1), status.double(),
                      root]).cpu().numpy()                                    # ... and everything per pose: the two read-backs
    cut = np.cumsum([0, 3 * M, 3 * M, 17 * M, 17 * M, M, M])
    h_trans, h_lin, h_err, h_err_lin, h_status, h_root = (flat[cut[k]:cut[k + 1]] for k in range(6))
    out = dict(raw)
    out['trans'], out['trans_linear'] = np.full((N, 3), np.nan), np.full((N, 3), np.nan)
    out['reproj_px'], out['reproj_px_linear'] = np.full((N, 17), np.nan, np.float32), np.full((N, 17), np.nan, np.float32)
    out['place_status'] = np.full(N, -1, np.int32)
    out['trans'][rows], out['trans_linear'][rows] = h_trans.reshape(M, 3), h_lin.reshape(M, 3)
    out['reproj_px'][rows], out['reproj_px_linear'][rows] = h_err.reshape(M, 17).astype(np.float32), h_err_lin.reshape(M, 17).astype(np.float32)
    out['place_status'][rows] = h_status.astype(np.int32)
    st = out['place_status'][rows]
    good = (st & place_report.BAD_BITS) == 0
    part = np.ones((M, 17), bool) if weights is None else (np.isfinite(weights.numpy()[rows]) & (weights.numpy()[rows] > 0))
    per_pose = np.array([h_err.reshape(M, 17)[i][part[i]].mean() for i in np.nonzero(good)[0]], dtype=np.float64)
    pose_error = {'n': int(per_pose.size), 'median': float(np.median(per_pose)) if per_pose.size else None,
                  'p95': float(np.percentile(per_pose, 95)) if per_pose.size else None}
    if root_err:
        out['root_err_mm'] = np.full(N, np.nan)
        out['root_err_mm'][rows] = h_root
        g_rows = gid[rows]
        for k, name in enumerate(names):
            table['groups'][name]['root_err_mm'] = _nanmean(h_root[good & (g_rows == k)])
        table[place_report.ALL]['root_err_mm'] = _nanmean(h_root[good])
    counts = {str(bit): int(((st & bit) != 0).sum()) for bit in place_report.STATUS_BITS}
    np.savez(os.path.join(directory, PLACE_NAME), **out)
    doc = place_report.write(directory, table, names, group_kind, n_iters, getattr(joints_of, 'name', None), weights_name, pose_error, counts, root_err)
    entry = {'source': os.path.basename(str(directory_or_npz)) if str(directory_or_npz).endswith('.npz') else 'refined.npz', 'placed': int(good.sum()),
             'rows': M, 'n_iters': n_iters, 'j_regressor': getattr(joints_of, 'name', None), 'weights': weights_name, 'status_counts': counts,
             'reproj_px_linear_mean': table[place_report.ALL]['reproj_linear_px'], 'reproj_px_mean': table[place_report.ALL]['reproj_px'],
             'pose_error_px': pose_error, 'depth_m_mean': table[place_report.ALL]['depth_m']}
    with open(os.path.join(directory, 'meta.json'), 'w') as f:
        json.dump(dict(meta, place=entry), f, indent=1, sort_keys=True, default=str)
    out['meta'] = dict(meta, place=entry)
    out['report'] = doc
    return out


def place_command(log=print) -> Optional[dict]:
    """`python main.py --place_refined PATH --data_root ROOT [--place_iters 10] [--place_weights FILE.npy] [--eval_j_regressor CKPT]`:
    refined.place on the split the table was written from -- its intrinsics and its full-frame gt_j2d, the groups of --eval_groups from
    its images.pkl.  One process: under torchrun rank 0 works and the other ranks return.  Prints one summary line."""
    from . import data as jdata, place_report
    if jdist.env_rank_world()[0] != 0:                      # the command joins no process group: the launcher's rank decides
        return None
    if not args.data_root:
        raise ValueError('--place_refined needs --data_root (the intrinsics and the 2-D joints of the split the table was written from)')
    if not 0 <= int(args.place_iters) <= PLACE_MAX_ITERS:
        raise ValueError(f'--place_iters {args.place_iters}: 0 .. {PLACE_MAX_ITERS}')
    location = jdata.split_location('validation', args.data_root)
    paths = jdata.split_image_paths(location)
    if paths is None:
        raise FileNotFoundError(f'--place_refined: {os.path.join(location, "images.pkl")} is missing: the frame paths say which group a sample belongs to')
    ds = jdata.data_set('validation', root=args.data_root)
    n_table = load_path(args.place_refined)['has_refined'].shape[0]
    if not (len(paths) == len(ds) == n_table):
        raise ValueError(f'--place_refined: the table holds {n_table} samples, the split {len(ds)} with {len(paths)} frame paths')
    weights = None
    if args.place_weights:
        weights = np.load(args.place_weights, allow_pickle=False)
        if weights.shape != (n_table, 17):
            raise ValueError(f'--place_weights {args.place_weights}: ({n_table}, 17) expected, got {weights.shape}')
    device = torch.device(args.device)
    torch.cuda.set_device(device)
    out = place(args.place_refined, ds.intrinsics, ds.gt_j2d, paths, _JointsOf(device), n_iters=args.place_iters, weights=weights,
                weights_name=args.place_weights, batch_size=args.batch_size, group_kind=args.eval_groups, gt_j3d_mm=ds.gt_j3d, device=device)
    directory = (os.path.dirname(args.place_refined) or '.') if str(args.place_refined).endswith('.npz') else args.place_refined
    log(place_report.summary_line(out['report']) + f'; {os.path.join(directory, PLACE_NAME)}')
    return out


# ---- what that camera sees (`--visible_refined`) ------------------------------------------------------------------------------
VISIBLE_NAME = 'refined_visible.npz'
VISIBLE_CODES = 'vertex_visibility.npy'
VISIBLE_PER_VERTEX = 'visible_per_vertex.npy'
VISIBLE_NO_POSE = 255         # vertex_visibility.npy / joint_code: a row without a refined or placed pose
VISIBLE_STATUS_BITS = {1: 'bit 0: the pose is left out of the report (not placed, a vertex or joint behind the camera, a non-finite error)'}


class _MeshOf(_JointsOf):
    """_JointsOf with the 6890 vertices beside the 17 joints: (joints (len(rows),17,3), verts (len(rows),6890,3)) on the device, neither
    translated; and the faces and skinning weights of the body it poses"""

    def __init__(self, device):
        super().__init__(device)
        self.faces = np.ascontiguousarray(np.asarray(self.smpl.model_np['faces']).astype(np.int32))
        self.lbs_weights = np.asarray(self.smpl.model_np['lbs_weights'])

    def __call__(self, arrays, rows):
        from . import engine as _engine
        B = int(len(rows))
        if B not in self.engines:
            self.engines[B] = _engine.RefineEngine(self.smpl.device_model, B, flags=_engine.FLAG_KEEP_VERTS)
            self.engines[B].set_j_regressor(self.J, self.mask)
        x6d = torch.from_numpy(arrays['pose6d'][rows]).to(self.device).float().contiguous()
        betas = torch.from_numpy(arrays['shape'][rows]).to(self.device).float().contiguous()
        return self.engines[B].find_joints_forward(betas, x6d=x6d, return_verts=True)


def visible_window(kind: str, n: int, frame=(1000, 1000), bboxes=None) -> torch.Tensor:
    """the window (n,4) float32 = [x0,y0,x1,y1] in full-frame pixels: the frame [0,0,W,H], or the square find_crop cuts from the
    sample's bounding box (data.crop_params: corner (min_x, min_y), side 1000 scale)"""
    from . import data as jdata
    if kind == 'frame':
        return torch.tensor([0.0, 0.0, float(frame[0]), float(frame[1])]).repeat(n, 1)
    if kind != 'crop':
        raise ValueError(f'visible: window {kind!r}: frame or crop')
    if bboxes is None or tuple(bboxes.shape) != (n, 4):
        raise ValueError(f'visible: the crop window needs bboxes ({n}, 4), got {None if bboxes is None else tuple(bboxes.shape)}')
    min_x, min_y, scale = jdata.crop_params(torch.as_tensor(bboxes).float())
    return torch.stack([min_x, min_y, min_x + 1000 * scale, min_y + 1000 * scale], 1).float()


def visible(directory_or_npz: str, intrinsics, gt_j3d_mm, paths, mesh_of, faces, part=None, n_parts: int = 0, margin_mm: float = 5.0,
            window: str = 'frame', frame=(1000, 1000), bboxes=None, batch_size: int = 256, group_kind: str = 'action', device=None) -> Dict[str, np.ndarray]:
    """`--visible_refined PATH`: what the real camera sees of every placed row of DIR/refined_placed.npz (PATH: that file, another `.npz`
    of the directory with `trans`, or the directory).  `mesh_of(arrays, rows)` gives (joints (len(rows),17,3), verts (len(rows),6890,3))
    of table rows on the device (_MeshOf); faces (n_faces,3) int32 and part (6890,) labels (or None) belong to that body.  Per chunk
    of `batch_size` refined rows: + (float)trans, jrr_point_visibility for the vertices (a face that names the vertex skipped, one
    crossing hides) and for the joints (two crossings hide: the first is the joint's own skin) against the window of `window` under the
    real intrinsics (N,3,3), jrr_evaluate_joints against the pelvis-centred gt_j3d_mm (N,17,3), jrr_visibility_accumulate into the
    table of visibility_report by the groups of `paths` (None: one group); nothing is read back inside the loop.  Writes
    DIR/vertex_visibility.npy -- uint8 (N,6890) codes (bit 0 hidden, bit 1 outside, bit 2 behind the camera), 255 on rows without a
    refined or placed pose, chunk by chunk through a memory map --, DIR/refined_visible.npz -- every array of the input unchanged +
    joint_code (N,17) uint8 (255 there), joint_crossings (N,17) int32 and n_vertices_seen (N,) int32 (-1 there), visible_status (N,)
    int32 (-1 there; bit 0: left out of the report) --, DIR/visible.json, DIR/visible.md, DIR/visible_per_vertex.npy (6890 int64: in
    how many counted poses the vertex is seen) and the entry `visible` of DIR/meta.json; the input file is not rewritten."""
    from . import engine as _engine, eval_report, utils, vertex_report, visibility_report
    margin_mm = float(margin_mm)
    if not (np.isfinite(margin_mm) and margin_mm >= 0.0):
        raise ValueError(f'visible: margin_mm {margin_mm}: finite and not negative')
    is_file = str(directory_or_npz).endswith('.npz')
    directory = (os.path.dirname(directory_or_npz) or '.') if is_file else directory_or_npz
    source = directory_or_npz if is_file else os.path.join(directory, PLACE_NAME)
    if not os.path.exists(source):
        raise FileNotFoundError(f'visible: {source} is missing: --place_refined writes it')
    raw = load_path(source)
    meta = raw.pop('meta')
    if 'trans' not in raw or 'place_status' not in raw:
        raise ValueError(f'visible: {source} holds no trans / place_status: run --place_refined on the table first')
    N = raw['has_refined'].shape[0]
    as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    intrinsics, gt_j3d_mm = as_t(intrinsics).float(), as_t(gt_j3d_mm).float()
    for name, t, shape in (('intrinsics', intrinsics, (N, 3, 3)), ('gt_j3d', gt_j3d_mm, (N, 17, 3))):
        if tuple(t.shape) != shape:
            raise ValueError(f'visible: {name} should be {shape} for a table of {N} samples, is {tuple(t.shape)}')
    rect_all = visible_window(window, N, frame, None if bboxes is None else as_t(bboxes))
    names, gid = eval_report.assign_groups(paths, group_kind, n=N)
    if gid.shape[0] != N:
        raise ValueError(f'visible: {gid.shape[0]} paths for a table of {N} rows')
    G = len(names)
    device = torch.device(args.device if device is None else device)
    faces_d = as_t(np.ascontiguousarray(np.asarray(faces).astype(np.int32))).to(device)
    part_np = None if part is None else np.ascontiguousarray(np.asarray(part).astype(np.int32))
    part_d = None if part_np is None else torch.from_numpy(part_np).to(device)
    rows = np.nonzero(raw['has_refined'])[0]
    M, bs = int(rows.size), max(1, int(batch_size))
    trans_all, pstatus_all = torch.from_numpy(raw['trans'][rows]), torch.from_numpy(raw['place_status'][rows].astype(np.int32))
    n_verts, vcode = None, None
    jcount = torch.zeros((M, 17), dtype=torch.int32, device=device)
    jcode = torch.full((M, 17), VISIBLE_NO_POSE, dtype=torch.uint8, device=device)
    n_seen = torch.full((M,), -1, dtype=torch.int32, device=device)
    left_out = torch.zeros((M,), dtype=torch.int32, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    acc = torch.zeros(G * visibility_report.ROW + visibility_report.TRAILER, dtype=torch.int64, device=device)
    per_vertex = None
    with torch.no_grad():
        for a in range(0, M, bs):
            idx = torch.from_numpy(rows[a:a + bs])
            s = slice(a, a + int(idx.shape[0]))
            joints, verts = mesh_of(raw, rows[a:a + bs])
            if vcode is None:                                                # the sizes of the body, from the first chunk
                n_verts = int(verts.shape[1])
                vcode = torch.full((M, n_verts), VISIBLE_NO_POSE, dtype=torch.uint8, device=device)
                per_vertex = torch.zeros(n_verts, dtype=torch.int64, device=device)
            t = trans_all[s].to(device).float()[:, None]
            verts_cam, joints_cam = (verts.float() + t).contiguous(), (joints.float() + t).contiguous()
            K, rect = intrinsics[idx].to(device).contiguous(), rect_all[idx].to(device).contiguous()
            _engine.point_visibility(verts_cam, faces_d, None, K, rect, margin_mm / 1000.0, 1, status, out=(None, vcode[s]))
            _engine.point_visibility(verts_cam, faces_d, joints_cam, K, rect, margin_mm / 1000.0, 2, status, out=(jcount[s], jcode[s]))
            gt = utils.move_pelvis(gt_j3d_mm[idx].to(device).float())
            err_mm = (_engine.evaluate_joints(joints.float().contiguous(), gt.contiguous())[0] * 1000).contiguous()
            pst = pstatus_all[s].to(device)
            _engine.visibility_accumulate(vcode[s], jcode[s], err_mm, part_d, pst, torch.from_numpy(gid[rows[a:a + bs]]).to(device), G, acc, per_vertex)
            n_seen[s] = (vcode[s] == 0).sum(1).int()
            left_out[s] = (((pst & 7) != 0) | ((vcode[s] & 0xFC) != 0).any(1) | ((jcode[s] & 0xFC) != 0).any(1) | ~(err_mm < 1.0e5).all(1)).int()
    if vcode is None:                                                        # a table without a refined row
        n_verts = 6890
        vcode = torch.zeros((0, n_verts), dtype=torch.uint8, device=device)
        per_vertex = torch.zeros(n_verts, dtype=torch.int64, device=device)
    table = visibility_report.derive(acc.cpu().numpy(), names)               # the table ...
    h_jcode, h_jcount, h_seen, h_left = jcode.cpu().numpy(), jcount.cpu().numpy(), n_seen.cpu().numpy(), left_out.cpu().numpy()
    placed = (raw['place_status'][rows] >= 0) & ((raw['place_status'][rows] & 7) == 0) & np.isfinite(raw['trans'][rows]).all(1)
    codes = np.lib.format.open_memmap(os.path.join(directory, VISIBLE_CODES), mode='w+', dtype=np.uint8, shape=(N, n_verts))
    codes[:] = VISIBLE_NO_POSE
    for a in range(0, M, bs):                                                # ... and the codes, chunk by chunk
        keep = placed[a:a + bs]
        codes[rows[a:a + bs][keep]] = vcode[a:a + bs].cpu().numpy()[keep]
    codes.flush()
    del codes
    np.save(os.path.join(directory, VISIBLE_PER_VERTEX), per_vertex.cpu().numpy())
    out = dict(raw)
    out['joint_code'] = np.full((N, 17), VISIBLE_NO_POSE, np.uint8)
    out['joint_crossings'] = np.full((N, 17), -1, np.int32)
    out['n_vertices_seen'] = np.full(N, -1, np.int32)
    out['visible_status'] = np.full(N, -1, np.int32)
    pr = rows[placed]
    out['joint_code'][pr], out['joint_crossings'][pr], out['n_vertices_seen'][pr] = h_jcode[placed], h_jcount[placed], h_seen[placed]
    out['visible_status'][rows] = h_left
    np.savez(os.path.join(directory, VISIBLE_NAME), **out)
    parts = None
    if part_np is not None:
        n_parts = int(n_parts) if n_parts else int(part_np.max()) + 1
        sizes = np.bincount(np.where((part_np >= 0) & (part_np < visibility_report.PARTS), part_np, visibility_report.PARTS - 1),
                            minlength=visibility_report.PARTS)
        parts = list(zip(vertex_report.part_names(min(n_parts, visibility_report.PARTS)), (int(x) for x in sizes)))
    face_status = int(status.item())
    doc = visibility_report.write(directory, table, names, group_kind, margin_mm, window, frame, getattr(mesh_of, 'name', None), parts, face_status)
    a_ = table[visibility_report.ALL]
    entry = {'source': os.path.basename(source), 'rows': M, 'placed': int(placed.sum()), 'counted': a_['n'], 'left_out': a_['n_bad'],
             'margin_mm': margin_mm, 'window': window, 'frame': [int(x) for x in frame], 'j_regressor': getattr(mesh_of, 'name', None),
             'vertices_seen': a_['vertices_seen'], 'vertices_occluded': a_['vertices_occluded'], 'vertices_outside': a_['vertices_outside'],
             'err_seen_mm': a_['err_seen_mm'], 'err_occluded_mm': a_['err_occluded_mm'], 'face_index_status': face_status}
    with open(os.path.join(directory, 'meta.json'), 'w') as f:
        json.dump(dict(meta, visible=entry), f, indent=1, sort_keys=True, default=str)
    out['meta'] = dict(meta, visible=entry)
    out['report'] = doc
    return out


def visible_command(log=print) -> Optional[dict]:
    """`python main.py --visible_refined PATH --data_root ROOT [--visible_margin_mm 5.0] [--visible_window frame|crop] [--visible_frame W H]
    [--eval_j_regressor CKPT]`: refined.visible on the split the table was written from -- its intrinsics, bounding boxes and gt_j3d, the
    groups of --eval_groups from its images.pkl.  One process: under torchrun rank 0 works and the other ranks return.  Prints one line."""
    from . import data as jdata, vertex_report, visibility_report
    if jdist.env_rank_world()[0] != 0:                      # the command joins no process group: the launcher's rank decides
        return None
    if not args.data_root:
        raise ValueError('--visible_refined needs --data_root (the intrinsics, the bounding boxes and the 3-D joints of the split the table was written from)')
    margin = float(args.visible_margin_mm)
    if not (np.isfinite(margin) and margin >= 0.0):
        raise ValueError(f'--visible_margin_mm {args.visible_margin_mm}: finite and not negative')
    if args.visible_window not in visibility_report.WINDOWS:
        raise ValueError(f'--visible_window {args.visible_window}: frame or crop')
    frame = [int(x) for x in args.visible_frame]
    if len(frame) != 2 or min(frame) < 1:
        raise ValueError(f'--visible_frame {args.visible_frame}: two positive numbers, W H')
    is_file = str(args.visible_refined).endswith('.npz')
    directory = (os.path.dirname(args.visible_refined) or '.') if is_file else args.visible_refined
    source = args.visible_refined if is_file else os.path.join(directory, PLACE_NAME)
    if not os.path.exists(source):
        raise FileNotFoundError(f'--visible_refined: {source} is missing: --place_refined writes it')
    head = load_path(source)
    if 'trans' not in head:
        raise ValueError(f'--visible_refined: {source} holds no trans: run --place_refined on the table first')
    location = jdata.split_location('validation', args.data_root)
    paths = jdata.split_image_paths(location)
    if paths is None:
        raise FileNotFoundError(f'--visible_refined: {os.path.join(location, "images.pkl")} is missing: the frame paths say which group a sample belongs to')
    ds = jdata.data_set('validation', root=args.data_root)
    n_table = head['has_refined'].shape[0]
    if not (len(paths) == len(ds) == n_table):
        raise ValueError(f'--visible_refined: the table holds {n_table} samples, the split {len(ds)} with {len(paths)} frame paths')
    device = torch.device(args.device)
    torch.cuda.set_device(device)
    mesh_of = _MeshOf(device)
    out = visible(source, ds.intrinsics, ds.gt_j3d, paths, mesh_of, mesh_of.faces, part=vertex_report.part_labels(mesh_of.lbs_weights),
                  n_parts=mesh_of.lbs_weights.shape[1], margin_mm=margin, window=args.visible_window, frame=frame, bboxes=ds.bboxes,
                  batch_size=args.batch_size, group_kind=args.eval_groups, device=device)
    log(visibility_report.summary_line(out['report']) + f'; {os.path.join(directory, VISIBLE_NAME)}')
    return out
