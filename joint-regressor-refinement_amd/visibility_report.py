"""The report of `--visible_refined` (refined.visible): what the real camera sees of the placed bodies, per group, joint and body part.

One int64 table by the report's groups (include/jrr.h, JRR_VIS_ACC_*: rows of 154 words + a 2-word trailer) that
jrr_visibility_accumulate fills on the device: poses counted and poses left out whole (not placed, a query behind the camera, a
non-finite error), the vertices seen / hidden behind the body / outside the window, per joint the poses in which it is seen, hidden
and outside with the sums of its 3-D error where seen and where hidden, and per body part the vertices seen against all.  `derive`
turns it into float64 numbers, `write` into visible.json / visible.md; both work on the host alone, as the other reports' do.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import eval_report, group_table
from .group_table import ALL, fmt as _fmt

LAYOUT_VERSION = 1            # include/jrr.h: JRR_VIS_ACC_LAYOUT_VERSION and the offsets below
ROW, TRAILER = 154, group_table.TRAILER
COUNT, BAD, SUM_VERT_SEEN, SUM_VERT_OCCLUDED, SUM_VERT_OUTSIDE = 0, 1, 2, 3, 4
J_SEEN, J_OCCLUDED, J_OUTSIDE, SUM_ERR_SEEN, SUM_ERR_OCCLUDED, PART_SEEN, PART_ALL = 5, 22, 39, 56, 73, 90, 122
NJ, PARTS = 17, 32
FIXED = float(1 << 24)        # the error sums are in units of 2^-24 mm
OCCLUDED, OUTSIDE, INVALID = 1, 2, 4      # JRR_VIS_*: the bits of a code
NO_POSE = 255                 # vertex_visibility.npy: a row without a refined or placed pose
CODE_BITS = {1: 'bit 0: hidden behind the body itself', 2: 'bit 1: the pixel lies outside the window',
             4: 'bit 2: behind the camera or not finite'}
WINDOWS = ('frame', 'crop')


def _share(a, b) -> Optional[float]:
    return float(a / b) if b else None


def _stats(row: np.ndarray) -> dict:
    n = int(row[COUNT])
    out = {'n': n, 'n_bad': int(row[BAD]), 'raw': [int(x) for x in row]}
    n_vert = float(row[PART_ALL:PART_ALL + PARTS].sum())                    # every vertex of every counted pose has one label
    for key, w in (('seen', SUM_VERT_SEEN), ('occluded', SUM_VERT_OCCLUDED), ('outside', SUM_VERT_OUTSIDE)):
        out[f'vertices_{key}'] = _share(float(row[w]), n_vert)
    for key, w in (('seen', J_SEEN), ('occluded', J_OCCLUDED), ('outside', J_OUTSIDE)):
        out[f'joints_{key}_n'] = [int(x) for x in row[w:w + NJ]]
        out[f'joints_{key}'] = [_share(float(x), n) for x in row[w:w + NJ]]
    for key, s0, n0 in (('seen', SUM_ERR_SEEN, J_SEEN), ('occluded', SUM_ERR_OCCLUDED, J_OCCLUDED)):
        sums, cnt = row[s0:s0 + NJ].astype(np.float64), row[n0:n0 + NJ].astype(np.float64)
        out[f'err_{key}_per_joint_mm'] = [float(s / FIXED / c) if c else None for s, c in zip(sums, cnt)]
        out[f'err_{key}_mm'] = float(sums.sum() / FIXED / cnt.sum()) if cnt.sum() else None
    out['parts_seen'] = [_share(float(s), float(a)) for s, a in zip(row[PART_SEEN:PART_SEEN + PARTS], row[PART_ALL:PART_ALL + PARTS])]
    return out


def derive(table: np.ndarray, names: Sequence[str]) -> dict:
    """the numbers of the int64 table (n_groups * 154 + 2 words), per group and for `all`, in float64: n, n_bad, the share of the
    vertices seen, occluded and outside, per joint the share of the poses in which it is seen, occluded (and inside) and outside, its
    mean 3-D error in mm where seen and where occluded, those means over all joints, and per part label the share of its vertices
    seen (None for a label without a vertex).  Raises when a pose carried a group id >= n_groups."""
    return group_table.derive(table, names, ROW, _stats, 'visibility table')


def _pct(x) -> str:
    return '-' if x is None else format(100.0 * x, '.1f')


def markdown(doc: dict) -> str:
    t = doc['table']
    lines = [f'# What the camera sees of the refined poses (groups by {doc["group_kind"]})', '',
             f'Regressor: {doc["j_regressor"]}.  Window: {doc["window"]}; a face hides a point when it crosses the ray from the camera centre more '
             f'than {doc["margin_mm"]:g} mm in front of it (a joint: the second such face, the first is its own skin).  Shares in %, errors in mm.', '',
             '| group | n | left out | vertices seen | hidden | outside | joint error seen | hidden |', '|---|---|---|---|---|---|---|---|']
    for name in list(doc['groups']) + [ALL]:
        r = t[ALL] if name == ALL else t['groups'][name]
        lines.append(f'| {name} | {r["n"]} | {r["n_bad"]} | {_pct(r["vertices_seen"])} | {_pct(r["vertices_occluded"])} | {_pct(r["vertices_outside"])} | '
                     f'{_fmt(r["err_seen_mm"])} | {_fmt(r["err_occluded_mm"])} |')
    a = t[ALL]
    lines += ['', 'Per joint, all groups:', '', '| joint | seen | hidden | outside | error seen | error hidden |', '|---|---|---|---|---|---|']
    for i, jn in enumerate(doc['joints']):
        lines.append(f'| {jn} | {_pct(a["joints_seen"][i])} | {_pct(a["joints_occluded"][i])} | {_pct(a["joints_outside"][i])} | '
                     f'{_fmt(a["err_seen_per_joint_mm"][i])} | {_fmt(a["err_occluded_per_joint_mm"][i])} |')
    if doc.get('parts'):
        lines += ['', 'Per body part, all groups (share of its vertices seen):', '', '| part | vertices | seen |', '|---|---|---|']
        for i, (pn, size) in enumerate(doc['parts']):
            lines.append(f'| {pn} | {size} | {_pct(a["parts_seen"][i])} |')
    if doc.get('face_index_status'):
        lines += ['', 'A face of the body model names a vertex outside the mesh; such faces hide nothing.']
    lines += ['', summary_line(doc)]
    return '\n'.join(lines) + '\n'


def summary_line(doc: dict) -> str:
    a = doc['table'][ALL]
    return (f'visibility of {a["n"]} poses ({doc["window"]} window, margin {doc["margin_mm"]:g} mm, {a["n_bad"]} left out): vertices seen '
            f'{_pct(a["vertices_seen"])} %, hidden {_pct(a["vertices_occluded"])} %, outside {_pct(a["vertices_outside"])} %; joint error seen '
            f'{_fmt(a["err_seen_mm"])} mm, hidden {_fmt(a["err_occluded_mm"])} mm')


def write(directory: str, table: dict, group_names: Sequence[str], group_kind: str, margin_mm: float, window: str, frame, j_regressor: Optional[str],
          parts, face_index_status: int) -> Optional[dict]:
    """DIR/visible.json and DIR/visible.md; rank 0 alone writes (the others return None).  parts: [(name, vertices)] or None."""
    doc = {'layout_version': LAYOUT_VERSION, 'group_kind': group_kind, 'groups': list(group_names), 'joints': list(eval_report.JOINT_NAMES),
           'table': table, 'margin_mm': float(margin_mm), 'window': window, 'frame': [int(x) for x in frame], 'j_regressor': j_regressor,
           'parts': None if parts is None else [[str(n), int(s)] for n, s in parts], 'face_index_status': int(face_index_status),
           'code_bits': {str(k): v for k, v in CODE_BITS.items()}}
    return group_table.write(directory, 'visible', doc, markdown)


def load(directory: str) -> dict:
    return group_table.load(directory, 'visible', LAYOUT_VERSION)
