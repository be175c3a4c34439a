"""The per-vertex error of meshes (`--eval_pve`): the fourth column of the evaluation report, PVE / MPVPE and its Procrustes-aligned form.

Definition (include/jrr.h, jrr_vertex_error): both meshes are root-centred (joint 0 of the INITIAL joint regressor on each), d_i is
the distance of vertex i, e_i the distance after the similarity fit of the whole predicted mesh to the target (the reference's
batch_compute_similarity_transform_torch on all 6890 vertices); PVE and PA-PVE of a pose are their means over the vertices, those of
a group the means over its poses.  No joint regressor is scored here: the retrained one plays no part.

`VertexReport` owns two int64 device tables (JRR_PVE_ACC_*: `n_groups` rows of 370 words + a 2-word trailer; 2 x 6890 per-vertex
sums).  `add()` is one launch and reads nothing back.  `finish()` makes ONE sum all-reduce of both tables under data parallelism
(exact: integers of disjoint shards), then the only read-back, and derives the numbers in float64: per group and for `all` n, n_bad,
PVE / PA-PVE in mm, the median and the 90th percentile of the per-pose values from the 1-mm histogram, the per-part means when the
vertices carry part labels (`--eval_pve_parts`: the argmax of the body model's skinning weights), and the per-vertex means.
`derive`, `markdown` and `write` work on numpy tables without a GPU.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import accel_report, group_table
from .group_table import ALL, fmt as _fmt

LAYOUT_VERSION = 1            # include/jrr.h: JRR_PVE_ACC_LAYOUT_VERSION and the offsets below
ROW, TRAILER, MAX_PARTS = 370, group_table.TRAILER, 32
COUNT, BAD, SUM, SUM_PA, HIST, HIST_PA, PART, PART_PA, BINS = 0, 1, 2, 3, 4, 155, 306, 338, 151
NV = 6890
FIXED = float(1 << 24)        # the sums are in units of 2^-24 m
GT_NAME = 'gt_vertices.npy'
PART_NAMES = ('Pelvis', 'L_Hip', 'R_Hip', 'Spine1', 'L_Knee', 'R_Knee', 'Spine2', 'L_Ankle', 'R_Ankle', 'Spine3', 'L_Foot', 'R_Foot', 'Neck',
              'L_Collar', 'R_Collar', 'Head', 'L_Shoulder', 'R_Shoulder', 'L_Elbow', 'R_Elbow', 'L_Wrist', 'R_Wrist', 'L_Hand', 'R_Hand')
_OWN_FLAGS = ('eval_pve', 'eval_pve_parts')


def check_flags(ns) -> None:
    """`--eval_pve` belongs to `--eval_vertices DIR --eval_report OUT`, `--eval_pve_parts` to `--eval_pve`"""
    if getattr(ns, 'eval_pve_parts', False) and not getattr(ns, 'eval_pve', False):
        raise ValueError('--eval_pve_parts needs --eval_pve')
    if getattr(ns, 'eval_pve', False) and not (ns.eval_vertices and ns.eval_report):
        raise ValueError('--eval_pve needs --eval_vertices DIR (with gt_vertices.npy) and --eval_report OUT (where pve.json / pve.md go)')


def flags_doc(flags: dict) -> dict:
    """the flags as the existing output files record them: `eval_pve` / `eval_pve_parts` change none of those files"""
    return {k: v for k, v in flags.items() if k not in _OWN_FLAGS}


def open_gt_vertices(directory: str, n: int):
    """the memmap of DIR/gt_vertices.npy, (n,6890,3) float32 metres; refuses -- with the file's name -- a missing file, a wrong shape
    or dtype.  NaN rows are allowed: their poses are counted as bad."""
    p = os.path.join(directory, GT_NAME)
    if not os.path.isfile(p):
        raise FileNotFoundError(f'--eval_pve: {p} is missing: the target meshes, ({n},6890,3) float32 metres')
    gt = np.load(p, mmap_mode='r')
    if gt.shape != (n, NV, 3):
        raise ValueError(f'{p}: ({n},6890,3) expected for {n} meshes, got {gt.shape}')
    if gt.dtype != np.float32:
        raise ValueError(f'{p}: float32 expected, got {gt.dtype}')
    return gt


def part_labels(lbs_weights: np.ndarray) -> np.ndarray:
    """(n_verts,) int32: the joint with the largest skinning weight of each vertex, the lowest index among equals"""
    W = np.asarray(lbs_weights)
    if W.ndim != 2 or not 1 <= W.shape[1] <= MAX_PARTS:
        raise ValueError(f'skinning weights: (n_verts, 1 .. {MAX_PARTS}) expected, got {W.shape}')
    return np.argmax(W, axis=1).astype(np.int32)         # numpy: the first occurrence of the maximum


def part_names(n_parts: int) -> list:
    return list(PART_NAMES[:n_parts]) + [f'part_{i}' for i in range(len(PART_NAMES), n_parts)]


# ---- the tables ----------------------------------------------------------------------------------------------------------------
class VertexReport:
    def __init__(self, group_names: Sequence[str], device, n_verts: int = NV, part: Optional[np.ndarray] = None, n_parts: int = 0):
        self.names = [str(g) for g in group_names]
        group_table.check_groups(len(self.names))
        self.device, self.n_verts = torch.device(device), int(n_verts)
        self.n_parts = int(n_parts) if part is not None else 0
        if part is not None:
            part = np.asarray(part)
            if part.shape != (self.n_verts,) or not 1 <= self.n_parts <= MAX_PARTS:
                raise ValueError(f'part labels: ({self.n_verts},) with 1 .. {MAX_PARTS} parts expected, got {part.shape} with {n_parts} parts')
        self.part_np = None if part is None else part.astype(np.int32)
        self.part = None if part is None else torch.from_numpy(self.part_np).to(self.device)
        G = len(self.names)
        self.both = torch.zeros(G * ROW + TRAILER + 2 * self.n_verts, dtype=torch.int64, device=self.device)      # one buffer: one all-reduce
        self.acc = self.both[:G * ROW + TRAILER]
        self.acc_v = self.both[G * ROW + TRAILER:].view(2, self.n_verts)

    def add(self, pred: torch.Tensor, gt: torch.Tensor, root_pred: Optional[torch.Tensor], root_gt: Optional[torch.Tensor],
            group_ids: Optional[torch.Tensor] = None) -> None:
        """pred, gt (B,n_verts,3) m, roots (B,3) or None, group_ids (B,) int32 on the same device (None: group 0); < 0 = do not score.
        One launch, nothing read back."""
        from . import engine as _engine
        _engine.vertex_error(pred, gt, root_pred, root_gt, group=group_ids, part=self.part, n_parts=self.n_parts, n_groups=len(self.names),
                             acc=self.acc, acc_v=self.acc_v, means=False, rows=False)

    def finish(self, reduce: bool = True) -> dict:
        """the ONE all-reduce (reduce=False: this process evaluated everything alone), the one read-back, the derivation"""
        host = group_table.all_reduce(self.both, reduce).cpu().numpy()
        cut = len(self.names) * ROW + TRAILER
        return derive(host[:cut], host[cut:].reshape(2, self.n_verts), self.names, self.part_np, self.n_parts)


def _stats(row: np.ndarray, parts) -> dict:
    n = int(row[COUNT])
    out = {'n': n, 'n_bad': int(row[BAD]), 'raw': [int(x) for x in row]}
    for key, s0, h0, p0 in (('pve', SUM, HIST, PART), ('pa_pve', SUM_PA, HIST_PA, PART_PA)):
        if n == 0:
            out.update({f'{key}_mm': None, f'{key}_median_mm': None, f'{key}_p90_mm': None})
            if parts is not None:
                out[f'{key}_per_part_mm'] = None
            continue
        out[f'{key}_mm'] = float(np.float64(row[s0]) / FIXED / n * 1000.0)
        hist = row[h0:h0 + BINS]
        out[f'{key}_median_mm'], out[f'{key}_p90_mm'] = accel_report.percentile_mm(hist, 0.5), accel_report.percentile_mm(hist, 0.9)
        if parts is not None:      # an empty part has no mean
            out[f'{key}_per_part_mm'] = {name: (float(np.float64(row[p0 + p]) / FIXED / n * 1000.0) if size else None) for p, (name, size) in enumerate(parts)}
    return out


def derive(table: np.ndarray, table_v: np.ndarray, names: Sequence[str], part: Optional[np.ndarray] = None, n_parts: int = 0) -> dict:
    """the numbers of the report from the int64 tables (n_groups * 370 + 2 words; (2,n_verts)): per group and for `all` n, n_bad, PVE /
    PA-PVE in mm = sum / 2^24 / n * 1000 in float64, the median and 90th percentile of the per-pose values from the histogram, the
    per-part means (part: the labels the table was filled with); `per_vertex_mm` (2,n_verts) float32 = table_v / 2^24 / n(all) * 1000
    (NaN without a counted pose).  Raises when a pose carried a group id >= n_groups."""
    rows, ignored = group_table.split(table, len(names), ROW, 'vertex error table')
    table_v = np.asarray(table_v)
    if table_v.dtype != np.int64 or table_v.ndim != 2 or table_v.shape[0] != 2:
        raise ValueError(f'per-vertex table: (2,n_verts) int64 expected, got {table_v.dtype} {table_v.shape}')
    parts = None
    if part is not None:
        sizes = np.bincount(np.asarray(part)[(np.asarray(part) >= 0) & (np.asarray(part) < n_parts)], minlength=n_parts)
        parts = list(zip(part_names(n_parts), (int(s) for s in sizes)))
    n_all = int(rows[:, COUNT].sum())
    per_vertex = (table_v.astype(np.float64) / FIXED / n_all * 1000.0).astype(np.float32) if n_all else np.full(table_v.shape, np.nan, dtype=np.float32)
    return {**group_table.assemble(rows, ignored, names, lambda row: _stats(row, parts)),
            'parts': None if parts is None else {name: size for name, size in parts}, 'per_vertex_mm': per_vertex}


# ---- the files -----------------------------------------------------------------------------------------------------------------
def markdown(doc: dict) -> str:
    lines = [f'# Per-vertex error ({doc["source"]}, groups by {doc["group_kind"]})', '',
             f'Errors in mm over the {doc["n_verts"]} vertices, both meshes centred at joint 0 of `{doc["j_regressor_initial"]["path"]}` '
             f'({doc["j_regressor_initial"]["sha256_16"]}); PA: after the similarity fit of the whole mesh.  Median and 90 % of the per-pose values.', '',
             '| group | n | bad | PVE | median | 90 % | PA-PVE | median | 90 % |', '|---|---|---|---|---|---|---|---|---|']
    for name in list(doc['groups']) + [ALL]:
        r = doc['data'][ALL] if name == ALL else doc['data']['groups'][name]
        lines.append(f'| {name} | {r["n"]} | {r["n_bad"]} | {_fmt(r["pve_mm"])} | {_fmt(r["pve_median_mm"])} | {_fmt(r["pve_p90_mm"])} | '
                     f'{_fmt(r["pa_pve_mm"])} | {_fmt(r["pa_pve_median_mm"])} | {_fmt(r["pa_pve_p90_mm"])} |')
    if doc['data'].get('parts'):
        r = doc['data'][ALL]
        lines += ['', 'Per body part, all groups (a vertex belongs to the joint with its largest skinning weight; the mean over the poses of the '
                  'part\'s mean):', '', '| part | vertices | PVE | PA-PVE |', '|---|---|---|---|']
        for name, size in doc['data']['parts'].items():
            a = None if r['pve_per_part_mm'] is None else r['pve_per_part_mm'][name]
            b = None if r['pa_pve_per_part_mm'] is None else r['pa_pve_per_part_mm'][name]
            lines.append(f'| {name} | {size} | {_fmt(a)} | {_fmt(b)} |')
    pv = doc.get('per_vertex')
    if pv:
        lines += ['', f'Per vertex (`{pv["file"]}`, (2,{doc["n_verts"]}) float32 mm: plain, aligned): largest mean {_fmt(pv["max_mm"][0])} at vertex '
                  f'{pv["argmax"][0]}, aligned {_fmt(pv["max_mm"][1])} at vertex {pv["argmax"][1]}.']
    if doc['data'].get('ignored'):
        lines += ['', f'{doc["data"]["ignored"]} samples were not scored (marked invalid by the dataset).']
    return '\n'.join(lines) + '\n'


def write(directory: str, result: dict, group_names: Sequence[str], group_kind: str, source: str, initial) -> Optional[dict]:
    """DIR/pve.json, DIR/pve.md and DIR/pve_per_vertex.npy from what finish() returned; rank 0 alone writes (the others return None).
    initial: (path, sha256[:16]) of the regressor whose joint 0 centred the meshes."""
    if group_table.rank() != 0:
        return None
    data = dict(result)
    per_vertex = np.asarray(data.pop('per_vertex_mm'), dtype=np.float32)
    finite = np.isfinite(per_vertex).all()
    doc = {'layout_version': LAYOUT_VERSION, 'source': source, 'group_kind': group_kind, 'groups': list(group_names), 'data': data,
           'n_verts': int(per_vertex.shape[1]), 'unit': 'mm', 'j_regressor_initial': {'path': initial[0], 'sha256_16': initial[1]},
           'per_vertex': {'file': 'pve_per_vertex.npy', 'max_mm': [float(v) for v in per_vertex.max(1)] if finite else [None, None],
                          'argmax': [int(v) for v in per_vertex.argmax(1)] if finite else [None, None]}}
    os.makedirs(directory, exist_ok=True)
    np.save(os.path.join(directory, 'pve_per_vertex.npy'), per_vertex)
    return group_table.write(directory, 'pve', doc, markdown)


def load(directory: str) -> dict:
    return group_table.load(directory, 'pve', LAYOUT_VERSION)


def summary_line(doc: dict) -> str:
    r = doc['data'][ALL]
    return f'per-vertex error, mm: PVE {_fmt(r["pve_mm"], ".4f")}  PA-PVE {_fmt(r["pa_pve_mm"], ".4f")} (n {r["n"]}, bad {r["n_bad"]})'
