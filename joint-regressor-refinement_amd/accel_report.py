"""The acceleration error along each video sequence (`--eval_accel`): the temporal column of the evaluation report.

Definition (include/jrr.h, jrr_accel_error; the HMMR / VIBE convention): a time order lists table rows; a position p whose listed
neighbours p - 1 and p + 1 belong to its run -- consecutive frames of one camera, as refined.sequence_runs forms runs -- is a triple.
With x = P - P[0] (prediction, m) and y = G / 1000 - (G / 1000)[0] (ground truth, mm) per frame, a = (x[p-1] - 2 x[p]) + x[p+1], and
e_j = |a_pred - a_gt| per joint.  The acceleration error of a set of positions is the mean of e_j over its triples and the 17 joints,
in metres per SAMPLED frame^2 (printed in mm); the runs' frame stride is recorded, because a dataset may be subsampled.

`JointTrack` holds `n_sets` prediction tables (n_rows,17,3) and one ground-truth table on the device, rows at dataset indices, and a
host-side `present` array.  `add()` scatters a batch with torch indexing and reads nothing back.  `finish()`: refined.sequence_runs on
the frame paths; under a process group ONE sum all-reduce of the float tables (the shards write disjoint rows of zero-filled tables, so
the sum is the union), then rank r takes dist.shard_bounds(M, r, world) of the positions; ONE jrr_accel_error launch per prediction
set into its own int64 table (include/jrr.h, JRR_ACCEL_ACC_*); ONE sum all-reduce of the int64 tables (exact); the one read-back;
`derive()` in float64.  `derive` and `write` work on CPU tensors, as eval_report's do.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import dist as jdist
from . import eval_report, group_table, refined
from .group_table import ALL

LAYOUT_VERSION = 1            # include/jrr.h: JRR_ACCEL_ACC_LAYOUT_VERSION and the offsets below
ROW, TRAILER = 205, group_table.TRAILER
COUNT, BAD, NO_TRIPLE, SUM_ERR, SUM_PRED, SUM_GT, HIST, BINS = 0, 1, 2, 3, 20, 37, 54, 151
NJ = 17
FIXED = float(1 << 24)        # the sums are in units of 2^-24 m per sampled frame^2
UNIT = 'mm per sampled frame^2'


def check_flags(ns) -> None:
    """`--eval_accel` with the evaluation commands needs `--eval_report DIR`; with --smooth_refined / --fuse_refined it needs nothing"""
    if getattr(ns, 'eval_accel', False) and not (ns.eval_report or ns.smooth_refined or ns.fuse_refined):
        raise ValueError('--eval_accel needs --eval_report DIR (where accel.json / accel.md go)')


def flags_doc(ns) -> dict:
    """the flags as the existing output files record them: `eval_accel` changes none of those files, so it is not among them"""
    return {k: v for k, v in vars(ns).items() if k != 'eval_accel'}


def read_paths(directory: str, n: int) -> List[str]:
    """the frame paths of an --eval_vertices directory: `paths.txt`, one line per mesh"""
    p = os.path.join(directory, 'paths.txt')
    if not os.path.isfile(p):
        raise ValueError(f'--eval_accel: {p} is missing: the frame paths say which meshes follow each other')
    with open(p) as f:
        paths = [line.rstrip('\n') for line in f]
    if len(paths) != n:
        raise ValueError(f'{p}: {len(paths)} lines for {n} meshes')
    return paths


class JointTrack:
    def __init__(self, n_rows: int, n_sets: int, device):
        self.n_rows, self.n_sets = int(n_rows), int(n_sets)
        if self.n_rows < 0 or self.n_sets < 1:
            raise ValueError(f'JointTrack: {n_rows} rows, {n_sets} sets')
        self.device = torch.device(device)
        self.flat = torch.zeros((self.n_sets + 1) * self.n_rows * NJ * 3, device=self.device)          # what finish() all-reduces
        tables = self.flat.view(self.n_sets + 1, self.n_rows, NJ, 3)
        self.pred, self.gt = tables[:self.n_sets], tables[self.n_sets]
        self.present = np.zeros(self.n_rows, dtype=bool)

    def add(self, index, joints_per_set: Sequence[torch.Tensor], gt_mm: torch.Tensor, valid=None) -> None:
        """rows `index` (B; a host array or CPU tensor of dataset indices: the host marks them present, the device copy scatters) <-
        the batch's joints (B,17,3) m of every set and its ground truth (B,17,3) mm.  `valid` (B, host, bool) or None: a sample the
        batch marks invalid is stored but not marked present.  Nothing is read back."""
        idx = np.asarray(index.cpu() if torch.is_tensor(index) else index).astype(np.int64).reshape(-1)
        B = idx.shape[0]
        if len(joints_per_set) != self.n_sets:
            raise ValueError(f'JointTrack.add: {len(joints_per_set)} sets of joints for a track of {self.n_sets}')
        if B and (idx.min() < 0 or idx.max() >= self.n_rows):
            raise ValueError(f'JointTrack.add: a dataset index outside [0, {self.n_rows})')
        d_idx = torch.from_numpy(idx).to(self.device, non_blocking=True)
        for s, joints in enumerate(joints_per_set):
            if joints.shape != (B, NJ, 3):
                raise ValueError(f'JointTrack.add: joints of set {s} should be ({B},17,3), are {tuple(joints.shape)}')
            self.pred[s][d_idx] = joints.detach().float()
        self.gt[d_idx] = gt_mm.detach().float().reshape(B, NJ, 3)
        ok = np.ones(B, dtype=bool) if valid is None else np.asarray(valid.cpu() if torch.is_tensor(valid) else valid).astype(bool).reshape(-1)
        self.present[idx[ok]] = True

    def finish(self, paths, group_ids: Optional[np.ndarray], names: Sequence[str], set_names: Sequence[str], reduce: bool = True,
               present: Optional[np.ndarray] = None) -> dict:
        """the document of the report (see module docstring).  paths: as refined.sequence_runs takes them; group_ids (n_rows,) int32 by
        dataset index or None (the single group); names: the groups; set_names: one per prediction table.  present: the whole split's
        present array where every rank knows it; without it the ranks' arrays are joined by one more small MAX all-reduce."""
        import torch.distributed as dist
        from . import engine as _engine
        names, set_names = [str(g) for g in names], [str(s) for s in set_names]
        G = len(names)
        if len(set_names) != self.n_sets:
            raise ValueError(f'JointTrack.finish: {len(set_names)} names for {self.n_sets} sets')
        group_table.check_groups(G)
        grouped = reduce and dist.is_available() and dist.is_initialized()
        rank, world = (dist.get_rank(), dist.get_world_size()) if grouped else (0, 1)
        have = self.present if present is None else np.asarray(present).astype(bool).reshape(-1)
        if have.shape != (self.n_rows,):
            raise ValueError(f'JointTrack.finish: present should be ({self.n_rows},), is {have.shape}')
        if grouped and present is None and world > 1:
            t = torch.from_numpy(have.astype(np.int32)).to(self.device)
            have = group_table.all_reduce(t, op=dist.ReduceOp.MAX).cpu().numpy().astype(bool)
        order, run, frame = refined.sequence_runs(paths, have)
        M = int(order.shape[0])
        group_table.all_reduce(self.flat, reduce, in_place=True)                      # THE float collective
        lo, hi = jdist.shard_bounds(M, rank, world)
        packed = torch.zeros(self.n_sets * (G * ROW + TRAILER) + 1, dtype=torch.int64, device=self.device)
        if hi > lo:
            d_order, d_run = torch.from_numpy(order).to(self.device), torch.from_numpy(run).to(self.device)
            d_group = None if group_ids is None else torch.from_numpy(np.asarray(group_ids).astype(np.int32)[order]).to(self.device)
            status = torch.zeros(1, dtype=torch.int32, device=self.device)
            for s in range(self.n_sets):
                acc = packed[s * (G * ROW + TRAILER):(s + 1) * (G * ROW + TRAILER)]
                _engine.accel_error(self.pred[s], self.gt, d_order, d_run, status, group=d_group, n_groups=G, acc=acc, begin=lo,
                                    count=hi - lo, rows=False)
            packed[-1:].copy_(status.long())
        host = group_table.all_reduce(packed, reduce).cpu().numpy()                   # THE integer collective and the one read-back
        if host[-1]:
            raise RuntimeError('acceleration error: an entry of the time order lies outside the table')
        tables = host[:-1].reshape(self.n_sets, G * ROW + TRAILER)
        return {'sets': {name: derive(tables[s], names) for s, name in enumerate(set_names)}, 'set_names': set_names, 'groups': names,
                'split': split_stats(run, frame), 'rows': self.n_rows, 'present': int(have.sum())}


def percentile_mm(hist: np.ndarray, q: float) -> Optional[float]:
    """the q-quantile of the values behind a 1-mm histogram (151 bins, the last one open), linear inside its bin; 150.0 stands for
    "150 mm or more"; None for an empty histogram"""
    hist = np.asarray(hist, dtype=np.float64)
    total = float(hist.sum())
    if total <= 0:
        return None
    cum = np.cumsum(hist)
    b = int(np.searchsorted(cum, q * total, side='left'))
    b = min(b, hist.shape[0] - 1)
    if b == hist.shape[0] - 1:
        return float(b)
    below = float(cum[b] - hist[b])
    return float(b + (q * total - below) / hist[b])


def _stats(row: np.ndarray) -> dict:
    n = int(row[COUNT])
    out = {'n': n, 'n_bad': int(row[BAD]), 'n_no_triple': int(row[NO_TRIPLE]), 'raw': [int(x) for x in row]}
    keys = (('accel_err', SUM_ERR), ('accel_pred', SUM_PRED), ('accel_gt', SUM_GT))
    if n == 0:
        out.update({f'{k}_mm': None for k, _ in keys})
        out.update({'accel_err_per_joint_mm': None, 'accel_err_median_mm': None, 'accel_err_p90_mm': None})
        return out
    for k, s0 in keys:
        sums = row[s0:s0 + NJ].astype(np.float64)
        out[f'{k}_mm'] = float(sums.sum() / FIXED / (NJ * n) * 1000.0)
        if k == 'accel_err':
            out['accel_err_per_joint_mm'] = [float(s / FIXED / n * 1000.0) for s in sums]
    hist = row[HIST:HIST + BINS]
    out['accel_err_median_mm'], out['accel_err_p90_mm'] = percentile_mm(hist, 0.5), percentile_mm(hist, 0.9)
    return out


def derive(table: np.ndarray, names: Sequence[str]) -> dict:
    """the numbers of one prediction set from its int64 table (n_groups * 205 + 2 words), per group and for `all`: n (triples scored),
    n_bad, n_no_triple, the acceleration error in mm = sum / 2^24 / (17 n) * 1000 in float64, its 17 per-joint means, the mean |a_pred|
    and |a_gt|, the median and the 90th percentile of e_j from the histogram.  Raises when a position carried a group id >= n_groups."""
    return group_table.derive(table, names, ROW, _stats, 'acceleration table', 'positions')


def split_stats(run: np.ndarray, frame: np.ndarray) -> dict:
    """what the split looks like along time: positions, runs, the histogram of run lengths, and of the frame stride of the runs of two or
    more positions (the difference of consecutive frame numbers, constant along a run)"""
    run, frame = np.asarray(run).astype(np.int64).reshape(-1), np.asarray(frame).astype(np.int64).reshape(-1)
    M = int(run.shape[0])
    if M == 0:
        return {'positions': 0, 'runs': 0, 'run_length_histogram': {}, 'stride_histogram': {}}
    lengths = np.bincount(run)
    lengths = lengths[lengths > 0]
    inside = run[1:] == run[:-1]
    first_step = inside & np.concatenate([[True], run[1:-1] != run[:-2]]) if M > 1 else np.zeros(0, dtype=bool)
    strides = (frame[1:] - frame[:-1])[first_step]
    lh, sh = np.unique(lengths, return_counts=True), np.unique(strides, return_counts=True)
    return {'positions': M, 'runs': int(lengths.shape[0]), 'run_length_histogram': {str(int(k)): int(c) for k, c in zip(*lh)},
            'stride_histogram': {str(int(k)): int(c) for k, c in zip(*sh)}}


def _fmt(x, spec='.3f') -> str:
    return group_table.fmt(x, spec)


def markdown(doc: dict) -> str:
    sets = doc['sets']
    first, last = doc['set_names'][0], doc['set_names'][-1]
    b, a = sets[first], sets[last]
    arrow = lambda key, rb, ra: f'{_fmt(rb[key])} → {_fmt(ra[key])}'
    sp = doc['split']
    lines = [f'# Acceleration error ({doc["source"]}, groups by {doc["group_kind"]})', '',
             f'{UNIT}, `{first}` → `{last}`; mean over the triples (a position with both neighbours in its run) and the 17 joints.  ',
             f'{sp["positions"]} positions in {sp["runs"]} runs; frame stride of the runs: '
             + (', '.join(f'{k} ({c} runs)' for k, c in sp['stride_histogram'].items()) or '-') + '.', '',
             '| group | triples | no triple | bad | accel error | median | 90 % | mean \\|a_pred\\| | mean \\|a_gt\\| |', '|---|---|---|---|---|---|---|---|---|']
    for name in list(doc['groups']) + [ALL]:
        rb = b[ALL] if name == ALL else b['groups'][name]
        ra = a[ALL] if name == ALL else a['groups'][name]
        lines.append(f'| {name} | {ra["n"]} | {ra["n_no_triple"]} | {ra["n_bad"]} | {arrow("accel_err_mm", rb, ra)} | '
                     f'{arrow("accel_err_median_mm", rb, ra)} | {arrow("accel_err_p90_mm", rb, ra)} | {arrow("accel_pred_mm", rb, ra)} | '
                     f'{_fmt(ra["accel_gt_mm"])} |')
    lines += ['', f'Per joint, all groups ({first} → {last} → difference; negative = `{last}` moves more like the ground truth):', '',
              '| joint | accel error |', '|---|---|']
    for i, jn in enumerate(doc['joints']):
        vb = None if b[ALL]['accel_err_per_joint_mm'] is None else b[ALL]['accel_err_per_joint_mm'][i]
        va = None if a[ALL]['accel_err_per_joint_mm'] is None else a[ALL]['accel_err_per_joint_mm'][i]
        diff = None if vb is None or va is None else va - vb
        lines.append(f'| {jn} | {_fmt(vb)} → {_fmt(va)} → {_fmt(diff, "+.3f")} |')
    lines += ['', 'Run lengths: ' + (', '.join(f'{k}: {c}' for k, c in sp['run_length_histogram'].items()) or '-') + '.']
    if a.get('ignored'):
        lines += ['', f'{a["ignored"]} positions were not scored (group < 0).']
    return '\n'.join(lines) + '\n'


def write(directory: str, result: dict, group_kind: str, source: str) -> Optional[dict]:
    """DIR/accel.json and DIR/accel.md from what finish() returned; rank 0 alone writes (the others return None)"""
    return group_table.write(directory, 'accel', lambda: dict(result, layout_version=LAYOUT_VERSION, source=source, group_kind=group_kind,
                                                              joints=list(eval_report.JOINT_NAMES), unit=UNIT), markdown)


def load(directory: str) -> dict:
    return group_table.load(directory, 'accel', LAYOUT_VERSION)


def summary_line(doc: dict) -> str:
    parts = []
    for name in doc['set_names']:
        r = doc['sets'][name][ALL]
        parts.append(f'{name} {_fmt(r["accel_err_mm"], ".4f")} (n {r["n"]}, no triple {r["n_no_triple"]}, bad {r["n_bad"]})')
    return f'acceleration error, {UNIT}: ' + '  '.join(parts)


def per_sample_mm(joint_sets: Sequence[torch.Tensor], gt_mm: torch.Tensor, paths, has) -> List[np.ndarray]:
    """per prediction table (N,17,3) the per-sample acceleration error in mm at dataset indices -- the mean over the 17 joints, NaN
    without a triple -- along the runs of the rows `has` marks (refined.sequence_runs).  One launch per table, one read-back."""
    from . import engine as _engine
    N, dev = int(gt_mm.shape[0]), gt_mm.device
    order, run, _ = refined.sequence_runs(paths, has)
    M = int(order.shape[0])
    out = [np.full(N, np.nan, dtype=np.float32) for _ in joint_sets]
    if M == 0:
        return out
    d_order, d_run = torch.from_numpy(order).to(dev), torch.from_numpy(run).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    means = []
    for joints in joint_sets:
        err_j, _, _ = _engine.accel_error(joints.contiguous(), gt_mm.contiguous(), d_order, d_run, status)
        means.append(err_j.mean(1) * 1000)
    host = torch.cat(means + [status.float()]).cpu().numpy()
    if host[-1]:
        raise RuntimeError('acceleration error: an entry of the time order lies outside the table')
    for k in range(len(joint_sets)):
        out[k][order] = host[k * M:(k + 1) * M]
    return out
