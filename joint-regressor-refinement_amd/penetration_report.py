"""The self-penetration of meshes (`--eval_penetration`): is a mesh a possible body at all.

Definition (include/jrr.h, jrr_mesh_winding / jrr_penetration_accumulate): every vertex x is pushed `offset` under the skin along its
vertex normal n (jrr_vertex_normals), p = x + t n with t = -s offset, s the sign of the signed volume sum a . (b x c) of the first
finite mesh (float64, on the host, once: the synthetic body's faces are wound inwards, nothing assumes +1).  The winding number w of
the closed surface around p is an integer: with k = rintf(|w|) a vertex is PENETRATING when k >= 2 (that piece of skin lies inside
another piece of the body), THIN when k == 0 (the body is thinner than the push), UNSURE when |w| is further than 0.1 from k (the
surface is not closed there, or the point lies on it).  No joint regressor is scored.

`PenetrationReport` owns one int64 device buffer -- the group table (JRR_PEN_ACC_*: `n_groups` rows of 55 words + a 2-word trailer) and
the per-vertex counts -- and the per-mesh counts n_pen / n_thin / n_unsure, int32 (3,N) at the rows of vertices.npy.  `add()` is
three launches (normals, winding numbers, accumulate) and one torch expression, and reads nothing back.  `finish()` sums both over the
ranks (exact: integers of disjoint shards), makes the only read-back and derives the numbers.  `derive`, `markdown`, `write` and
`load` work on numpy tables without a GPU.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import group_table, vertex_report
from .group_table import ALL, fmt as _fmt

LAYOUT_VERSION = 1            # include/jrr.h: JRR_PEN_ACC_LAYOUT_VERSION and the offsets below
ROW, TRAILER, BINS, MAX_PARTS = 55, group_table.TRAILER, 16, 32
COUNT, BAD, POSES_PEN, POSES_PEN8, SUM_PEN, SUM_THIN, SUM_UNSURE, HIST, PART = 0, 1, 2, 3, 4, 5, 6, 7, 23
NV = 6890
WORST = 20
_OWN_FLAGS = ('eval_penetration', 'eval_penetration_offset_mm')
HIST_LABELS = ['0', '1'] + [f'{1 << (b - 1)}-{(1 << b) - 1}' for b in range(2, BINS - 1)] + [f'>={1 << (BINS - 2)}']


def check_flags(ns) -> None:
    """`--eval_penetration` belongs to `--eval_vertices DIR --eval_report OUT`, needs a body model and an offset in (0, 10] mm"""
    if not getattr(ns, 'eval_penetration', False):
        return
    if not (ns.eval_vertices and ns.eval_report):
        raise ValueError('--eval_penetration needs --eval_vertices DIR (the meshes) and --eval_report OUT (where penetration.json / '
                         'penetration.md go)')
    off = float(ns.eval_penetration_offset_mm)
    if not (math.isfinite(off) and 0.0 < off <= 10.0):
        raise ValueError(f'--eval_penetration_offset_mm {ns.eval_penetration_offset_mm}: a finite push with 0 < MM <= 10 expected')
    from . import regressor_report
    if not regressor_report.body_model_available(ns.smpl_dir, ns.synthetic):
        raise ValueError('--eval_penetration needs the body model (its faces, skinning weights and parents): --smpl_dir with '
                         'SMPL_NEUTRAL.npz / .pkl, or --synthetic')


def flags_doc(flags) -> dict:
    """the flags as the existing output files record them: the `eval_penetration*` flags change none of those files"""
    flags = flags if isinstance(flags, dict) else vars(flags)
    return {k: v for k, v in flags.items() if k not in _OWN_FLAGS}


def orientation(verts, faces) -> int:
    """+1 / -1: the sign of the signed volume sum a . (b x c) of the first finite mesh of verts (N,n_verts,3), in float64.  +1: the faces
    are wound outwards and so point the vertex normals.  Raises on a volume of zero and on a table without a finite mesh."""
    f = np.asarray(faces).astype(np.int64)
    for i in range(verts.shape[0]):
        v = np.asarray(verts[i], dtype=np.float64)
        if not np.isfinite(v).all():
            continue
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        vol = float(np.einsum('fc,fc->', a, np.cross(b, c)))
        if vol == 0.0:
            raise ValueError(f'--eval_penetration: mesh {i} has a signed volume of zero: its faces do not say which side is inside')
        return 1 if vol > 0 else -1
    raise ValueError('--eval_penetration: no mesh with finite vertices')


# ---- the tables ----------------------------------------------------------------------------------------------------------------
class PenetrationReport:
    def __init__(self, group_names: Sequence[str], device, faces: np.ndarray, n_total: int, offset_mm: float, sign: int,
                 part: Optional[np.ndarray] = None, n_parts: int = 0, n_verts: int = NV):
        self.names = [str(g) for g in group_names]
        group_table.check_groups(len(self.names))
        if sign not in (1, -1):
            raise ValueError(f'orientation {sign!r}: +1 or -1')
        self.device, self.n_verts, self.n_total = torch.device(device), int(n_verts), int(n_total)
        self.offset_mm, self.sign = float(offset_mm), int(sign)
        self.t = -self.sign * (self.offset_mm / 1000.0)
        self.n_parts = int(n_parts) if part is not None else 0
        if part is not None:
            part = np.asarray(part)
            if part.shape != (self.n_verts,) or not 1 <= self.n_parts <= MAX_PARTS:
                raise ValueError(f'part labels: ({self.n_verts},) with 1 .. {MAX_PARTS} parts expected, got {part.shape} with {n_parts} parts')
        self.part_np = None if part is None else part.astype(np.int32)
        self.part = None if part is None else torch.from_numpy(self.part_np).to(self.device)
        self.faces_np = np.ascontiguousarray(np.asarray(faces).astype(np.int32))
        self.faces = torch.from_numpy(self.faces_np).to(self.device)
        G = len(self.names)
        self.both = torch.zeros(G * ROW + TRAILER + self.n_verts, dtype=torch.int64, device=self.device)      # one buffer: one all-reduce
        self.acc = self.both[:G * ROW + TRAILER]
        self.acc_v = self.both[G * ROW + TRAILER:]
        self.counts = torch.zeros((3, self.n_total), dtype=torch.int32, device=self.device)      # n_pen, n_thin, n_unsure; a rank fills its rows
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)

    def add(self, verts: torch.Tensor, group_ids: Optional[torch.Tensor], first: int) -> None:
        """verts (B,n_verts,3) m on the device: the meshes of rows first .. first + B of the table; group_ids (B,) int32 (None: group
        0), < 0 = do not score.  Three launches, nothing read back."""
        from . import engine as _engine, report
        B = int(verts.shape[0])
        if not 0 <= first <= first + B <= self.n_total:
            raise ValueError(f'rows {first} .. {first + B} of {self.n_total}')
        normals = report.vertex_normals(verts, self.faces_np)
        points = verts + self.t * normals
        wind = _engine.mesh_winding(verts, self.faces, points, self.status)
        rows = [self.counts[k, first:first + B] for k in range(3)]
        _engine.penetration_accumulate(wind, self.part, group_ids, len(self.names), self.acc, self.acc_v, *rows)

    def finish(self, reduce: bool = True) -> dict:
        """the sums over the ranks (reduce=False: this process evaluated everything alone), the one read-back, the derivation"""
        host, counts = (group_table.all_reduce(t, reduce).cpu().numpy() for t in (self.both, self.counts))
        if int(self.status.item()) & 1:
            raise RuntimeError('--eval_penetration: a face of the body model names a vertex outside the mesh')
        cut = len(self.names) * ROW + TRAILER
        out = derive(host[:cut], host[cut:], self.names, self.part_np, self.n_parts)
        out['counts'] = counts
        return out


def _stats(row: np.ndarray, parts, n_verts: int) -> dict:
    n = int(row[COUNT])
    out = {'n': n, 'n_bad': int(row[BAD]), 'poses_pen': int(row[POSES_PEN]), 'poses_pen8': int(row[POSES_PEN8]),
           'hist': [int(x) for x in row[HIST:HIST + BINS]], 'raw': [int(x) for x in row]}
    share = lambda x, d: (float(np.float64(x) / d) if d else None)
    out['share_pen'], out['share_pen8'] = share(row[POSES_PEN], n), share(row[POSES_PEN8], n)
    out['mean_n_pen'] = share(row[SUM_PEN], n)
    out['share_thin'], out['share_unsure'] = share(row[SUM_THIN], n * n_verts), share(row[SUM_UNSURE], n * n_verts)
    if parts is not None:
        out['per_part'] = {name: int(row[PART + p]) for p, (name, _) in enumerate(parts)}
    return out


def derive(table: np.ndarray, per_vertex: np.ndarray, names: Sequence[str], part: Optional[np.ndarray] = None, n_parts: int = 0) -> dict:
    """the numbers of the report from the int64 tables (n_groups * 55 + 2 words; (n_verts,)): per group and for `all` n, n_bad, the
    poses and the share of poses with any and with at least 8 penetrating vertices, the mean and the histogram of n_pen, the share of
    thin and of unsure vertices (of n * n_verts), the penetrating vertices per part (part: the labels the table was filled with).
    Raises when a pose carried a group id >= n_groups."""
    rows, ignored = group_table.split(table, len(names), ROW, 'penetration table')
    per_vertex = np.asarray(per_vertex)
    if per_vertex.dtype != np.int64 or per_vertex.ndim != 1:
        raise ValueError(f'per-vertex table: (n_verts,) int64 expected, got {per_vertex.dtype} {per_vertex.shape}')
    parts = None
    if part is not None:
        p = np.asarray(part)
        sizes = np.bincount(p[(p >= 0) & (p < n_parts)], minlength=n_parts)
        parts = list(zip(vertex_report.part_names(n_parts), (int(s) for s in sizes)))
    nv = int(per_vertex.shape[0])
    return {**group_table.assemble(rows, ignored, names, lambda row: _stats(row, parts, nv)),
            'parts': None if parts is None else {name: size for name, size in parts}, 'per_vertex': per_vertex.copy()}


def worst_poses(counts: np.ndarray, k: int = WORST) -> list:
    """the k meshes with the most penetrating vertices, by dataset index: the largest n_pen first, the smaller index among equals;
    meshes without a penetrating vertex are not listed"""
    counts = np.asarray(counts)
    order = np.lexsort((np.arange(counts.shape[1]), -counts[0].astype(np.int64)))[:k]
    return [{'index': int(i), 'n_pen': int(counts[0, i]), 'n_thin': int(counts[1, i]), 'n_unsure': int(counts[2, i])} for i in order if counts[0, i] > 0]


# ---- the files -----------------------------------------------------------------------------------------------------------------
def _pct(x) -> str:
    return '-' if x is None else format(100.0 * x, '.2f')


def markdown(doc: dict) -> str:
    lines = [f'# Self-penetration ({doc["source"]}, groups by {doc["group_kind"]})', '',
             f'Every one of the {doc["n_verts"]} vertices pushed {doc["offset_mm"]:g} mm under the skin along its normal (faces wound: winding '
             f'{doc["orientation"]:+d} inside); k = the rounded winding number of the whole surface around it.  Penetrating: k >= 2, that piece '
             'of skin lies inside another piece of the body.  Thin: k = 0, the body is thinner than the push.  Unsure: further than 0.1 from an '
             'integer.  A few penetrating vertices can be mesh noise: the second share asks for 8.', '',
             '| group | n | bad | poses >= 1 | % | poses >= 8 | % | mean n_pen | thin % | unsure % |', '|---|---|---|---|---|---|---|---|---|---|']
    for name in list(doc['groups']) + [ALL]:
        r = doc['data'][ALL] if name == ALL else doc['data']['groups'][name]
        lines.append(f'| {name} | {r["n"]} | {r["n_bad"]} | {r["poses_pen"]} | {_pct(r["share_pen"])} | {r["poses_pen8"]} | {_pct(r["share_pen8"])} | '
                     f'{_fmt(r["mean_n_pen"])} | {_pct(r["share_thin"])} | {_pct(r["share_unsure"])} |')
    r = doc['data'][ALL]
    lines += ['', 'Poses by their number of penetrating vertices, all groups:', '', '| n_pen | ' + ' | '.join(HIST_LABELS) + ' |',
              '|---|' + '---|' * BINS, '| poses | ' + ' | '.join(str(x) for x in r['hist']) + ' |']
    if doc['data'].get('parts'):
        lines += ['', 'Penetrating vertices per body part, all groups (a vertex belongs to the joint with its largest skinning weight; summed '
                  'over the poses):', '', '| part | vertices | penetrating | per pose |', '|---|---|---|---|']
        for name, size in doc['data']['parts'].items():
            c = r['per_part'][name]
            lines.append(f'| {name} | {size} | {c} | {_fmt(c / r["n"] if r["n"] else None)} |')
    if doc.get('worst'):
        lines += ['', f'The {len(doc["worst"])} worst meshes (row of vertices.npy):', '', '| index | n_pen | n_thin | n_unsure |', '|---|---|---|---|']
        lines += [f'| {w["index"]} | {w["n_pen"]} | {w["n_thin"]} | {w["n_unsure"]} |' for w in doc['worst']]
    pv = doc['per_vertex']
    lines += ['', f'Per vertex (`{pv["file"]}`, ({doc["n_verts"]},) int64: the poses in which the vertex penetrates): {pv["n_ever"]} vertices penetrate in '
              f'some pose, vertex {pv["argmax"]} most often ({pv["max"]} poses).  Per mesh: `{doc["per_mesh"]["file"]}` (n_pen, n_thin, n_unsure).']
    if doc['data'].get('ignored'):
        lines += ['', f'{doc["data"]["ignored"]} samples were not scored (marked invalid by the dataset).']
    return '\n'.join(lines) + '\n'


def write(directory: str, result: dict, group_names: Sequence[str], group_kind: str, source: str, offset_mm: float, sign: int) -> Optional[dict]:
    """DIR/penetration.json, DIR/penetration.md, DIR/penetration_per_vertex.npy and DIR/penetration.npz from what finish() returned;
    rank 0 alone writes (the others return None)"""
    if group_table.rank() != 0:
        return None
    data = dict(result)
    per_vertex = np.asarray(data.pop('per_vertex'), dtype=np.int64)
    counts = np.asarray(data.pop('counts'), dtype=np.int32)
    doc = {'layout_version': LAYOUT_VERSION, 'source': source, 'group_kind': group_kind, 'groups': list(group_names), 'data': data,
           'n_verts': int(per_vertex.shape[0]), 'offset_mm': float(offset_mm), 'orientation': int(sign), 'hist_labels': HIST_LABELS,
           'worst': worst_poses(counts),
           'per_vertex': {'file': 'penetration_per_vertex.npy', 'n_ever': int((per_vertex > 0).sum()), 'max': int(per_vertex.max(initial=0)),
                          'argmax': int(per_vertex.argmax()) if per_vertex.size else None},
           'per_mesh': {'file': 'penetration.npz', 'n': int(counts.shape[1])}}
    os.makedirs(directory, exist_ok=True)
    np.save(os.path.join(directory, 'penetration_per_vertex.npy'), per_vertex)
    np.savez(os.path.join(directory, 'penetration.npz'), n_pen=counts[0], n_thin=counts[1], n_unsure=counts[2])
    return group_table.write(directory, 'penetration', doc, markdown)


def load(directory: str) -> dict:
    return group_table.load(directory, 'penetration', LAYOUT_VERSION)


def summary_line(doc: dict) -> str:
    r = doc['data'][ALL]
    return (f'self-penetration ({doc["offset_mm"]:g} mm push): {_pct(r["share_pen"])} % of the poses penetrate, {_pct(r["share_pen8"])} % with 8 '
            f'vertices or more; mean {_fmt(r["mean_n_pen"])} vertices; thin {_pct(r["share_thin"])} %, unsure {_pct(r["share_unsure"])} % '
            f'(n {r["n"]}, bad {r["n_bad"]})')
