"""The report of `--place_refined` (refined.place): how well the placed bodies meet their 2-D annotation, per group and per joint.

One int64 table by the report's groups (include/jrr.h, JRR_PLACE_ACC_*: rows of 55 words + a 2-word trailer) that
jrr_place_accumulate fills on the device: poses counted, poses without a translation (status bits 0 .. 2), poses in which a
Levenberg-Marquardt step met a failed pivot (bit 3), the sum of the depths, and per joint the number of poses in which it took part
with the sums of its pixel distance after the linear start and at the result.  `derive` turns it into float64 numbers, `write` into
place.json / place.md; both work on the host alone, as the other reports' do.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import eval_report, group_table
from .group_table import ALL, arrow as _arrow, fmt as _fmt

LAYOUT_VERSION = 1            # include/jrr.h: JRR_PLACE_ACC_LAYOUT_VERSION and the offsets below
ROW, TRAILER = 55, group_table.TRAILER
COUNT, BAD, STEP_PIVOT, SUM_TZ, JOINTS, SUM_ERR_LIN, SUM_ERR = 0, 1, 2, 3, 4, 21, 38
NJ = 17
FIXED = float(1 << 24)        # the sums are in units of 2^-24 m or px
STATUS_BITS = {1: 'bit 0: fewer than 2 taking-part joints, or a non-finite input', 2: 'bit 1: the linear start is singular',
               4: 'bit 2: the linear start puts a taking-part joint behind the camera', 8: 'bit 3: a step met a failed pivot (the result is kept)'}
BAD_BITS = 7


def _stats(row: np.ndarray) -> dict:
    n = int(row[COUNT])
    out = {'n': n, 'n_bad': int(row[BAD]), 'n_step_pivot': int(row[STEP_PIVOT]), 'raw': [int(x) for x in row]}
    part = row[JOINTS:JOINTS + NJ].astype(np.float64)
    out['joints_n'] = [int(x) for x in row[JOINTS:JOINTS + NJ]]
    out['depth_m'] = float(row[SUM_TZ] / FIXED / n) if n else None
    for key, s0 in (('reproj_linear', SUM_ERR_LIN), ('reproj', SUM_ERR)):
        sums = row[s0:s0 + NJ].astype(np.float64)
        out[f'{key}_per_joint_px'] = [float(s / FIXED / p) if p else None for s, p in zip(sums, part)]
        out[f'{key}_px'] = float(sums.sum() / FIXED / part.sum()) if part.sum() else None
    return out


def derive(table: np.ndarray, names: Sequence[str]) -> dict:
    """the numbers of the int64 table (n_groups * 55 + 2 words), per group and for `all`, in float64: n, n_bad, n_step_pivot, the mean
    depth trans_z in m, per joint the number of poses it took part in and its mean pixel distance after the linear start and at the
    result, and those means over all taking-part joints.  Raises when a pose carried a group id >= n_groups."""
    return group_table.derive(table, names, ROW, _stats, 'place table')


def markdown(doc: dict) -> str:
    t = doc['table']
    lines = [f'# Camera-frame translation of the refined poses (groups by {doc["group_kind"]})', '',
             f'Regressor: {doc["j_regressor"]}.  {doc["n_iters"]} Levenberg-Marquardt steps behind the linear start; weights: {doc["weights"] or "ones"}.  '
             'Pixel distance of the placed joints from the 2-D annotation in full-frame pixels, linear start → result.', '',
             '| group | n | no translation | failed pivot | depth m | reprojection px |' + (' pelvis mm |' if doc.get('root_err') else ''),
             '|---|---|---|---|---|---|' + ('---|' if doc.get('root_err') else '')]
    for name in list(doc['groups']) + [ALL]:
        r = t[ALL] if name == ALL else t['groups'][name]
        root = f' {_fmt(r.get("root_err_mm"))} |' if doc.get('root_err') else ''
        lines.append(f'| {name} | {r["n"]} | {r["n_bad"]} | {r["n_step_pivot"]} | {_fmt(r["depth_m"], ".3f")} | '
                     f'{_arrow(r["reproj_linear_px"], r["reproj_px"], ".3f")} |{root}')
    lines += ['', 'Per joint, all groups:', '', '| joint | poses | reprojection px |', '|---|---|---|']
    a = t[ALL]
    for i, jn in enumerate(doc['joints']):
        lines.append(f'| {jn} | {a["joints_n"][i]} | {_arrow(a["reproj_linear_per_joint_px"][i], a["reproj_per_joint_px"][i], ".3f")} |')
    p = doc['pose_error_px']
    lines += ['', f'Per-pose mean pixel distance: median {_fmt(p["median"], ".3f")}, 95th percentile {_fmt(p["p95"], ".3f")} ({p["n"]} poses).']
    if doc.get('status_counts'):
        lines += [''] + [f'{c} poses: {STATUS_BITS[int(bit)]}.' for bit, c in sorted(doc['status_counts'].items(), key=lambda kv: int(kv[0])) if c]
    lines += ['', summary_line(doc)]
    return '\n'.join(lines) + '\n'


def summary_line(doc: dict) -> str:
    a, p = doc['table'][ALL], doc['pose_error_px']
    root = f', pelvis {_fmt(a.get("root_err_mm"))} mm from the measured one' if doc.get('root_err') else ''
    return (f'placed {a["n"]} poses ({doc["n_iters"]} steps, {a["n_bad"]} without a translation, {a["n_step_pivot"]} with a failed pivot): '
            f'reprojection {_arrow(a["reproj_linear_px"], a["reproj_px"], ".4f")} px, median {_fmt(p["median"], ".4f")}, 95 % {_fmt(p["p95"], ".4f")}, '
            f'mean depth {_fmt(a["depth_m"], ".3f")} m{root}')


def write(directory: str, table: dict, group_names: Sequence[str], group_kind: str, n_iters: int, j_regressor: str, weights: Optional[str],
          pose_error_px: dict, status_counts: dict, root_err: bool) -> Optional[dict]:
    """DIR/place.json and DIR/place.md; rank 0 alone writes (the others return None)"""
    doc = {'layout_version': LAYOUT_VERSION, 'group_kind': group_kind, 'groups': list(group_names), 'joints': list(eval_report.JOINT_NAMES),
           'table': table, 'n_iters': int(n_iters), 'j_regressor': j_regressor, 'weights': weights, 'pose_error_px': pose_error_px,
           'status_counts': status_counts, 'status_bits': {str(k): v for k, v in STATUS_BITS.items()}, 'root_err': bool(root_err)}
    return group_table.write(directory, 'place', doc, markdown)


def load(directory: str) -> dict:
    return group_table.load(directory, 'place', LAYOUT_VERSION)
