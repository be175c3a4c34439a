"""The regressor report (`--regressor_report DIR`): what the retrained J_regressor did to each H36M joint.

The artefact of the reference is a retrained regressor; its figure (teaser.png) shows the fitted mesh with the joints of the "currently
accepted" regressor in green, of the retrained one in blue and the ground truth in red.  /root/reference/scripts/test.py:107-123
regresses both sets of joints and keeps only their errors.  This module keeps the difference of the two sets:

`ShiftReport` owns an int64 device table (include/jrr.h, JRR_SHIFT_ACC_*: `n_groups` rows of 1277 words + a 2-word trailer).  `add()` is
one launch (jrr_regressor_shift_accumulate: per pose the displacement of every joint in a frame fixed to the body, integer atomics)
and reads nothing back; `finish()` makes ONE sum-all-reduce under data parallelism (exact: integers of disjoint shards), then the only
read-back, and `derive()` turns the table into numbers in float64.  `finish`, `derive` and `write` work on a CPU tensor with a gloo
group as well.

`compare_regressors()` is the part that needs no data: per joint the supports of both regressors, their overlap, the L1 distance of
the normalised rows, the heaviest vertices and the shift on the template body.

`Pictures` renders what the numbers describe (it needs a body model: faces for the rasteriser): pose_%05d.png, the shaded body front |
side with A's joints in green, B's in blue and the ground truth in red (jrr_draw_discs over jrr_mesh_shade, framed by
report.frame_camera), and weights_%02d_<Joint>.png, the template body with discs at the support vertices of A (green) and B (blue),
radius 1.5 + 6 sqrt(weight) pixels, and the two regressed joints in the pale colours on top.

`DepthReport` (`--regressor_report_depth`) asks what the displacement cannot say: is a joint still under the skin?  A row of the regressor
lies on the simplex, so its joint lies in the convex hull of its support vertices -- and the hull of a hand and a thigh vertex is mostly
air.  Per batch one jrr_point_mesh_depth on the vertices with 51 points per pose (the joints of A, of B, and the ground truth placed at A's
pelvis as in `Pictures.pose_pictures`), then one jrr_depth_accumulate into an int64 table (include/jrr.h, JRR_DEPTH_ACC_*); `finish()` is one
sum-all-reduce and one read-back, `derive_depth()` the numbers, `write_depth()` DIR/depth.json and DIR/depth.md.  The other files keep
their bytes.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import bones_report, ci_report, eval_protocol, penetration_report
from . import args as jargs
from . import group_table
from .eval_report import JOINT_NAMES, sha16
from .group_table import ALL, fmt as _f, rank as _rank

LAYOUT_VERSION = 1            # include/jrr.h: JRR_SHIFT_ACC_LAYOUT_VERSION and the offsets below
ROW, TRAILER = 1277, group_table.TRAILER
COUNT, BAD, SUM, MOM, ABS, ABS_REL, HIST, BINS = 0, 1, 2, 53, 155, 172, 189, 64
NJ = 17
FIXED = float(1 << 24)        # lengths are in units of 2^-24 m, the moments in units of 2^-32 m^2
BIN_MM = 2.0
GREEN, BLUE, RED = (0, 200, 0), (0, 0, 255), (255, 0, 0)
PALE_GREEN, PALE_BLUE = (160, 255, 160), (160, 160, 255)
JOINT_RADIUS_WEIGHTS = 4.0    # pixels, the regressed joints of the weight pictures
MAX_DISCS = 256               # include/jrr.h: JRR_DISCS_MAX_POINTS -- a longer support is drawn by its heaviest vertices
TOP = 5


# ---- the table -------------------------------------------------------------------------------------------------------------
class ShiftReport:
    def __init__(self, group_names: Sequence[str], device):
        self.names = [str(g) for g in group_names]
        group_table.check_groups(len(self.names))
        self.device = torch.device(device)
        self.acc = torch.zeros(len(self.names) * ROW + TRAILER, dtype=torch.int64, device=self.device)

    def add(self, joints_a: torch.Tensor, joints_b: torch.Tensor, group_ids: Optional[torch.Tensor] = None) -> None:
        """joints of the initial (a) and the retrained (b) regressor on the same meshes, (B,17,3) m as regressed; group_ids (B,) int32 on
        the same device (None: group 0), < 0 = do not score.  One launch, nothing read back."""
        from . import engine as _engine
        if group_ids is not None and (group_ids.device != joints_a.device or group_ids.dtype != torch.int32):
            raise ValueError(f'ShiftReport.add: group_ids must be an int32 tensor on {joints_a.device}, got {group_ids.dtype} on '
                             f'{group_ids.device}')
        _engine.regressor_shift_accumulate(joints_a.detach().float(), joints_b.detach().float(), group_ids, len(self.names), self.acc)

    def finish(self, reduce: bool = True) -> dict:
        """the ONE all-reduce (reduce=False: this process saw everything alone), the one read-back, the derivation"""
        return derive(group_table.all_reduce(self.acc, reduce).cpu().numpy(), self.names)


def _quantile_mm(hist: np.ndarray, n: int, p: float) -> float:
    """upper edge in mm of the first bin at which the cumulated histogram reaches p * n; the open last bin (>= 126 mm) reports its
    nominal edge, 128 mm"""
    k = int(np.searchsorted(np.cumsum(hist.astype(np.float64)), p * n, side='left'))
    return float((min(k, BINS - 1) + 1) * BIN_MM)


def _stats(row: np.ndarray) -> dict:
    n, n_bad = int(row[COUNT]), int(row[BAD])
    out = {'n': n, 'n_bad': n_bad, 'raw': [int(x) for x in row]}
    keys = ('mean_mm', 'std_mm', 'mean_abs_mm', 'mean_abs_pelvis_relative_mm', 'median_abs_mm', 'p95_abs_mm')
    if n == 0:
        out.update({k: None for k in keys})
        return out
    s = row[SUM:SUM + NJ * 3].astype(np.float64).reshape(NJ, 3) / n                       # mean of q, units of 2^-24 m
    m = row[MOM:MOM + NJ * 6].astype(np.float64).reshape(NJ, 6)[:, [0, 3, 5]]             # xx, yy, zz: sums of floor(q q / 2^16)
    # every term lost the fraction of its division by 2^16: the variance reads up to 2^-32 m^2 low, never high, and is clamped at zero --
    # poses that all moved alike have exactly no spread
    var = np.maximum(m * 65536.0 / n - s * s, 0.0)
    hist = row[HIST:HIST + NJ * BINS].reshape(NJ, BINS)
    out['mean_mm'] = (s / FIXED * 1000.0).tolist()
    out['std_mm'] = (np.sqrt(var) / FIXED * 1000.0).tolist()
    out['mean_abs_mm'] = (row[ABS:ABS + NJ].astype(np.float64) / FIXED / n * 1000.0).tolist()
    out['mean_abs_pelvis_relative_mm'] = (row[ABS_REL:ABS_REL + NJ].astype(np.float64) / FIXED / n * 1000.0).tolist()
    out['median_abs_mm'] = [_quantile_mm(hist[j], n, 0.5) for j in range(NJ)]
    out['p95_abs_mm'] = [_quantile_mm(hist[j], n, 0.95) for j in range(NJ)]
    return out


def derive(table: np.ndarray, names: Sequence[str]) -> dict:
    """the numbers of the int64 table (n_groups * 1277 + 2 words), per group and for `all`, in float64, per joint: the mean displacement
    in the body frame (mm; x to the body's left, y up, z forward) = sum / 2^24 / n * 1000 and its per-axis standard deviation from the
    second moments (a moment word drops up to 2^-32 m^2 per pose: a spread below ~0.015 mm may read as zero, one of a millimetre reads
    up to 1e-4 mm low), the mean |d|, the mean pelvis-relative |d|, the median and the 95th percentile of |d| from the 2-mm histogram (bin
    upper edges), n and n_bad.  Raises when a pose carried a group id >= n_groups."""
    return group_table.derive(table, names, ROW, _stats, 'regressor-shift table', verb='counted')


# ---- the depth below the skin ------------------------------------------------------------------------------------------------
DEPTH_LAYOUT_VERSION = 1      # include/jrr.h: JRR_DEPTH_ACC_LAYOUT_VERSION and the offsets below
D_ROW, D_OUTSIDE, D_UNSURE, D_SUM, D_HIST, D_BINS, D_COLS = 4290, 2, 66, 130, 194, 64, 64
D_BIN_MM, D_LOW_MM = 4.0, -64.0
DEPTH_SETS = ('initial', 'retrained', 'ground_truth')      # point columns 0..16, 17..33, 34..50
DEPTH_KEYS = ('mean_mm', 'outside', 'unsure', 'median_mm', 'p05_mm')


class DepthReport:
    """the int64 table of the depth section and the faces it is measured against, on one device"""

    def __init__(self, group_names: Sequence[str], device, faces):
        self.names = [str(g) for g in group_names]
        group_table.check_groups(len(self.names))
        faces = np.asarray(faces)
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
            raise ValueError(f'depth section: faces (n_faces,3) expected, got {faces.shape}')
        self.device = torch.device(device)
        self.faces = torch.from_numpy(np.ascontiguousarray(faces.astype(np.int32))).to(self.device)
        self.acc = torch.zeros(len(self.names) * D_ROW + TRAILER, dtype=torch.int64, device=self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)

    def add(self, verts: torch.Tensor, joints_a: torch.Tensor, joints_b: torch.Tensor, gt_centred_mm: torch.Tensor,
            group_ids: Optional[torch.Tensor] = None) -> None:
        """verts (B,V,3) m; joints_a / joints_b (B,17,3) m as regressed on them; gt_centred_mm (B,17,3) pelvis-centred, placed at A's
        pelvis; group_ids (B,) int32 on the device (None: group 0).  Two launches, nothing read back."""
        from . import engine as _engine
        ja = joints_a.detach().float()
        points = torch.cat([ja, joints_b.detach().float(), gt_centred_mm.detach().float() / 1000.0 + ja[:, :1]], dim=1).contiguous()
        dist, wind, _ = _engine.point_mesh_depth(verts.detach().float(), self.faces, points, self.status, want_face=False)
        _engine.depth_accumulate(dist, wind, group_ids, len(self.names), self.acc)

    def finish(self, reduce: bool = True) -> dict:
        """the ONE all-reduce (the status word rides behind the table), the one read-back, the derivation"""
        table = group_table.all_reduce(torch.cat([self.acc, self.status.to(torch.int64)]), reduce).cpu().numpy()
        if int(table[-1]) != 0:
            raise RuntimeError('depth section: a face of the body model names a vertex outside the meshes; it was skipped (status bit 0)')
        return derive_depth(table[:-1], self.names)


def _depth_quantile_mm(hist: np.ndarray, n: int, p: float) -> float:
    """upper edge in mm of the first 4-mm bin at which the cumulated histogram reaches p * n; bin 0 (everything below -60 mm) reports
    -60, the open last bin (>= 188 mm) its nominal edge, 192"""
    k = int(np.searchsorted(np.cumsum(hist.astype(np.float64)), p * n, side='left'))
    return float(D_LOW_MM + (min(k, D_BINS - 1) + 1) * D_BIN_MM)


def _depth_stats(row: np.ndarray, n_sets: int) -> dict:
    n, n_bad = int(row[COUNT]), int(row[BAD])
    out = {'n': n, 'n_bad': n_bad, 'sets': {}}
    hist = row[D_HIST:D_HIST + D_COLS * D_BINS].reshape(D_COLS, D_BINS)
    for s in range(n_sets):
        cols = slice(s * NJ, (s + 1) * NJ)
        if n == 0:
            out['sets'][DEPTH_SETS[s]] = {k: None for k in DEPTH_KEYS}
            continue
        out['sets'][DEPTH_SETS[s]] = {
            'mean_mm': (row[D_SUM:D_SUM + D_COLS][cols].astype(np.float64) / FIXED / n * 1000.0).tolist(),
            'outside': (row[D_OUTSIDE:D_OUTSIDE + D_COLS][cols].astype(np.float64) / n).tolist(),
            'unsure': (row[D_UNSURE:D_UNSURE + D_COLS][cols].astype(np.float64) / n).tolist(),
            'median_mm': [_depth_quantile_mm(hist[k], n, 0.5) for k in range(s * NJ, (s + 1) * NJ)],
            'p05_mm': [_depth_quantile_mm(hist[k], n, 0.05) for k in range(s * NJ, (s + 1) * NJ)]}
    return out


def derive_depth(table: np.ndarray, names: Sequence[str], n_sets: int = 3) -> dict:
    """the numbers of the int64 table (n_groups * 4290 + 2 words), per group and for `all`, in float64, for each set (point columns
    17 s .. 17 s + 16) and joint: the mean signed depth in mm (positive: under the skin) = sum / 2^24 / n * 1000, the share of poses in
    which the joint is outside, the share in which the winding number is no integer within 0.1, the median and the 5th percentile of the
    depth from the 4-mm histogram (bin upper edges), n and n_bad.  Raises when a pose carried a group id >= n_groups."""
    if not 1 <= n_sets <= D_COLS // NJ:
        raise ValueError(f'depth table: {n_sets} sets of {NJ} columns: 1 .. {D_COLS // NJ}')
    return group_table.derive(table, names, D_ROW, lambda row: _depth_stats(row, n_sets), 'depth table', verb='counted')


def template_depth(model_np: Dict[str, np.ndarray], J_a, J_b, mask, device) -> dict:
    """both regressors' joints on v_template, which needs no data: one launch of batch 1 with 34 points, read back.  Per regressor and
    joint the signed depth in mm, the winding number and the nearest face; `orientation`: the sign of the windings of the points inside
    (0: none is inside)"""
    from . import engine as _engine
    vt = np.asarray(model_np['v_template'], dtype=np.float32)
    pts = np.concatenate([normalised(J, mask) @ vt.astype(np.float64) for J in (J_a, J_b)]).astype(np.float32)
    dev = torch.device(device)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    faces = torch.from_numpy(np.ascontiguousarray(np.asarray(model_np['faces']).astype(np.int32))).to(dev)
    dist, wind, face = _engine.point_mesh_depth(torch.from_numpy(vt[None]).to(dev), faces, torch.from_numpy(pts[None]).to(dev), status)
    dist, wind, face = dist.cpu().numpy()[0].astype(np.float64), wind.cpu().numpy()[0].astype(np.float64), face.cpu().numpy()[0]
    if int(status.item()) != 0:
        raise RuntimeError('depth section: a face of the body model names a vertex outside v_template (status bit 0)')
    inside = np.abs(wind) > 0.5
    depth = np.where(inside, dist, -dist) * 1000.0
    out = {'orientation': int(np.sign(wind[inside].sum())) if inside.any() else 0}
    for s, name in enumerate(DEPTH_SETS[:2]):
        k = slice(s * NJ, (s + 1) * NJ)
        out[name] = {'depth_mm': depth[k].tolist(), 'wind': wind[k].tolist(), 'face': [int(f) for f in face[k]]}
    return out


def newly_outside(data: dict) -> List[int]:
    """the joints that the retrained regressor puts outside the body in some pose and the initial one in none (over all groups)"""
    sets = data[ALL]['sets']
    if sets['retrained']['outside'] is None:
        return []
    return [j for j in range(NJ) if sets['retrained']['outside'][j] > 0 and sets['initial']['outside'][j] == 0]


def depth_markdown(doc: dict) -> str:
    data, tpl = doc['data'], doc['template']
    orient = {1: 'outward normals by the right-hand rule (winding +1 inside)', -1: 'inward normals by the right-hand rule (winding -1 inside)',
              0: 'unknown (no template joint is inside)'}[tpl['orientation']]
    lines = [f'# Depth of the joints below the skin ({doc["source"]})', '',
             'Signed distance from each joint to the nearest point of the mesh surface, in mm: positive under the skin, negative outside.  '
             'Inside and outside come from the winding number of the surface around the point, not from face normals.', '',
             f'Mesh orientation: {orient}.', '',
             f'{data[ALL]["n"]} poses ({data[ALL]["n_bad"]} with a non-finite value or beyond the cap, {data["ignored"]} not scored).', '']
    flagged = doc['newly_outside']
    if flagged:
        lines += ['**Joints the retrained regressor puts outside the body in some pose and the initial one in none: ' +
                  ', '.join(JOINT_NAMES[j] for j in flagged) + '.**', '']
    else:
        lines += ['No joint is outside the body under the retrained regressor alone.', '']
    for name, title in zip(DEPTH_SETS, ('A, the initial regressor', 'B, the retrained regressor', 'The ground truth, placed at A\'s pelvis')):
        r = data[ALL]['sets'][name]
        lines += [f'## {title}', '', '| joint | mean | median | 5th percentile | outside % | unsure % | on the template |', '|---|---|---|---|---|---|---|']
        for j in range(NJ):
            g = lambda key: None if r[key] is None else r[key][j]
            pct = lambda key: '-' if r[key] is None else format(100.0 * r[key][j], '.2f')
            t = _f(tpl[name]['depth_mm'][j]) if name in tpl else '-'
            mark = ' **!**' if name == 'retrained' and j in flagged else ''
            lines.append(f'| {JOINT_NAMES[j]}{mark} | {_f(g("mean_mm"))} | {_f(g("median_mm"), ".0f")} | {_f(g("p05_mm"), ".0f")} | {pct("outside")} | '
                         f'{pct("unsure")} | {t} |')
        lines.append('')
    lines += ['Share of poses with the retrained regressor\'s joint outside, per group, %:', '', '| group | n | ' + ' | '.join(JOINT_NAMES) + ' |',
              '|---|---|' + '---|' * NJ]
    for name in doc['groups']:
        r = data['groups'][name]
        o = r['sets']['retrained']['outside']
        cells = ['-'] * NJ if o is None else [format(100.0 * x, '.1f') for x in o]
        lines.append(f'| {name} | {r["n"]} | ' + ' | '.join(cells) + ' |')
    return '\n'.join(lines) + '\n'


def write_depth(directory: str, data: dict, template: dict, group_names: Sequence[str], source: str, body_model: Optional[str]) -> Optional[dict]:
    """DIR/depth.json and DIR/depth.md; rank 0 alone writes (the others return None)"""
    doc = lambda: {'layout_version': DEPTH_LAYOUT_VERSION, 'source': source, 'groups': list(group_names), 'joint_names': list(JOINT_NAMES),
           'sets': list(DEPTH_SETS), 'bin_mm': D_BIN_MM, 'bin_low_mm': D_LOW_MM, 'orientation': template['orientation'],
           'sign': 'depth > 0: under the skin; inside <=> |winding number| > 0.5', 'data': data, 'template': template,
           'newly_outside': newly_outside(data), 'body_model': body_model}
    return group_table.write(directory, 'depth', doc, depth_markdown)


def load_depth(directory: str) -> dict:
    return group_table.load(directory, 'depth', DEPTH_LAYOUT_VERSION, 'depth table')


# ---- the two regressors, without data ----------------------------------------------------------------------------------------
def normalised(J, mask=None) -> np.ndarray:
    """J*mask -> ReLU -> each row divided by its sum (scripts/utils.py:87-92), float64 of the float32 inputs; an empty row stays zero"""
    J = np.asarray(J, dtype=np.float32).astype(np.float64)
    if mask is not None:
        J = J * np.asarray(mask, dtype=np.float32).astype(np.float64)
    J = np.maximum(J, 0.0)
    s = J.sum(axis=1, keepdims=True)
    return np.divide(J, s, out=np.zeros_like(J), where=s > 0)


def _top(row: np.ndarray) -> List[dict]:
    order = np.lexsort((np.arange(row.size), -row))[:TOP]
    return [{'vertex': int(v), 'weight': float(row[v])} for v in order if row[v] > 0]


def compare_regressors(J_a, J_b, mask=None, v_template=None) -> List[dict]:
    """per joint: support sizes (positive entries after mask, ReLU and row normalisation) of A and B, the vertices in both, the L1
    distance of the normalised rows, the five heaviest vertices of each and -- with a template (6890,3) -- the shift
    (Jn_B - Jn_A) @ v_template in mm, all in float64 on the host"""
    A, B = normalised(J_a, mask), normalised(J_b, mask)
    if A.shape != B.shape or A.ndim != 2 or A.shape[0] != NJ:
        raise ValueError(f'regressors: two (17,V) arrays expected, got {A.shape} and {B.shape}')
    shift = None
    if v_template is not None:
        shift = (B - A) @ np.asarray(v_template, dtype=np.float64) * 1000.0
    rows = []
    for j in range(NJ):
        rows.append({'joint': JOINT_NAMES[j], 'support_a': int((A[j] > 0).sum()), 'support_b': int((B[j] > 0).sum()),
                     'shared': int(((A[j] > 0) & (B[j] > 0)).sum()), 'l1': float(np.abs(A[j] - B[j]).sum()),
                     'top_a': _top(A[j]), 'top_b': _top(B[j]),
                     'template_shift_mm': None if shift is None else shift[j].tolist()})
    return rows


# ---- the pictures ------------------------------------------------------------------------------------------------------------
def project_points(points: torch.Tensor, cam: torch.Tensor, size: int) -> torch.Tensor:
    """points (B,P,3) in SMPL space under the rasteriser's projection (include/jrr.h, jrr_mesh_shade step 1) with cam (B,3), as pixel
    coordinates (x = column, y = row) of a size x size picture whose pixel (i, j) has its centre at NDC (1 - (2j + 1) / size,
    1 - (2i + 1) / size): (B,P,2) float32"""
    S = float(int(size))
    F = 5000.0 / S
    X = -2.0 * points[..., 0] + cam[:, None, 0]
    Y = -2.0 * points[..., 1] + cam[:, None, 1]
    Z = 2.0 * points[..., 2] + cam[:, None, 2]
    u, v = F * X / Z, F * Y / Z
    return torch.stack([((1.0 - u) * S - 1.0) * 0.5, ((1.0 - v) * S - 1.0) * 0.5], dim=-1).float()


def pose_disc_radius(size: int) -> float:
    return 3.0 * int(size) / 256.0


class Pictures:
    """shaded front and side views of bodies with discs painted over them; `model_np`: the body model's arrays (faces, v_template),
    `device_model`: engine.DeviceModel of it"""

    def __init__(self, model_np: Dict[str, np.ndarray], device_model, size: int):
        from . import engine as _engine
        if int(size) % 32 or not 32 <= int(size) <= 256:
            raise ValueError(f'--regressor_report_size {size}: a size the rasteriser takes, a multiple of 32 up to 256')
        if model_np.get('faces') is None:
            raise ValueError('regressor report pictures: the body model has no faces')
        self.model_np, self.device_model, self.size = model_np, device_model, int(size)
        self.flags = _engine.FLAG_KEEP_VERTS | _engine.FLAG_SILHOUETTE | (0 if self.size == 224 else _engine.FLAG_SIL_SIZE(self.size))
        self._engines = {}

    def _engine(self, n: int):
        from . import engine as _engine
        if n not in self._engines:
            self._engines[n] = _engine.RefineEngine(self.device_model, n, flags=self.flags)
        return self._engines[n]

    def views(self, verts: torch.Tensor, points: Sequence[torch.Tensor]):
        """verts (n,6890,3), points: tensors (n,P,3) of the same bodies.  Returns (front, side, front_xy, side_xy): the shaded views
        uint8 (n,S,S,3) -- the front over black, the body turned as report.side_view turns it over grey -- each framed by
        report.frame_camera, and per entry of `points` its pixel coordinates (n,P,2) in either view"""
        from . import report as _report
        S = self.size
        verts = verts.detach().float().contiguous()
        n = verts.shape[0]
        eng, faces = self._engine(n), self.model_np['faces']
        centre = verts.mean(dim=1, keepdim=True)
        cam_f = _report.frame_camera(verts, S).contiguous()
        eng.silhouette_forward(verts, cam_f)
        front = _report.mesh_shade(verts, cam_f, eng.silhouette_pix_to_face(), faces)
        turned = _report.side_view(verts, cam_f).contiguous()
        cam_s = _report.frame_camera(turned, S).contiguous()
        eng.silhouette_forward(turned, cam_s)
        side = _report.mesh_shade(turned, cam_s, eng.silhouette_pix_to_face(), faces, background=_report.SIDE_GREY)
        front_xy = [project_points(p.float(), cam_f, S) for p in points]
        side_xy = [project_points(_report.side_view(p.float(), cam_f, centre=centre), cam_s, S) for p in points]
        return front, side, front_xy, side_xy

    def pose_pictures(self, verts, joints_a, joints_b, gt_m) -> torch.Tensor:
        """(n,S,2S,3) uint8: front | side, A's joints green, B's blue, then the ground truth red (gt_m (n,17,3): pelvis-centred, metres,
        placed at A's pelvis)"""
        from . import engine as _engine
        gt = gt_m.float() + joints_a[:, :1].float()
        front, side, fxy, sxy = self.views(verts, [joints_a, joints_b, gt])
        r = pose_disc_radius(self.size)
        _engine.draw_discs(front, torch.stack(fxy).contiguous(), [GREEN, BLUE, RED], radius=r)
        _engine.draw_discs(side, torch.stack(sxy).contiguous(), [GREEN, BLUE, RED], radius=r)
        return torch.cat([front, side], dim=2)

    def weight_layers(self, J_a, J_b, mask=None):
        """what the weight pictures are made of: (front, side, front_xy, side_xy, radii, colours) -- the unpainted template views
        (17,S,S,3), the disc centres (4,17,P,2) per view and radii (4,17,P) of the sets {support of A, support of B, joint of A, joint of
        B} (NaN where a set has fewer than P points), the sets' colours.  Picture j belongs to joint j."""
        dev = self.device_model.device
        A, B = normalised(J_a, mask), normalised(J_b, mask)
        vt = np.asarray(self.model_np['v_template'], dtype=np.float64)
        P = int(max(1, min(MAX_DISCS, max(int((A > 0).sum(1).max()), int((B > 0).sum(1).max())))))
        pts = np.full((4, NJ, P, 3), np.nan, dtype=np.float32)
        rad = np.full((4, NJ, P), np.nan, dtype=np.float32)
        for k, Jn in enumerate((A, B)):
            for j in range(NJ):
                idx = np.flatnonzero(Jn[j] > 0)
                idx = idx[np.lexsort((idx, -Jn[j][idx]))][:P][::-1]        # heaviest last: painted on top
                pts[k, j, :idx.size] = vt[idx]
                rad[k, j, :idx.size] = 1.5 + 6.0 * np.sqrt(Jn[j][idx])
                pts[2 + k, j, 0] = Jn[j] @ vt
                rad[2 + k, j, 0] = JOINT_RADIUS_WEIGHTS if Jn[j].any() else np.nan
        verts = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(vt.astype(np.float32), (NJ, vt.shape[0], 3)))).to(dev)
        sets = [torch.from_numpy(pts[k]).to(dev) for k in range(4)]
        front, side, fxy, sxy = self.views(verts, sets)
        return front, side, torch.stack(fxy).contiguous(), torch.stack(sxy).contiguous(), torch.from_numpy(rad).to(dev), \
            [GREEN, BLUE, PALE_GREEN, PALE_BLUE]

    def weight_pictures(self, J_a, J_b, mask=None) -> torch.Tensor:
        """(17,S,2S,3) uint8: the template body front | side, picture j with the support of joint j"""
        from . import engine as _engine
        front, side, fxy, sxy, rad, colours = self.weight_layers(J_a, J_b, mask)
        _engine.draw_discs(front, fxy, colours, radii=rad)
        _engine.draw_discs(side, sxy, colours, radii=rad)
        return torch.cat([front, side], dim=2)


class PoseKeeper:
    """the first `n` scored poses this process sees: vertices, both joint sets and the centred ground truth in metres, kept on the device"""

    def __init__(self, n: int):
        self.n, self.kept = max(0, int(n)), []

    def have(self) -> int:
        return sum(int(k[0].shape[0]) for k in self.kept)

    def offer(self, verts, joints_a, joints_b, gt_centred_mm, scored: Optional[np.ndarray] = None) -> None:
        """scored: host booleans (B,), None = all; no device value is read"""
        want = self.n - self.have()
        if want <= 0:
            return
        B = int(verts.shape[0])
        idx = np.flatnonzero(np.ones(B, dtype=bool) if scored is None else np.asarray(scored, dtype=bool))[:want]
        if idx.size == 0:
            return
        sel = torch.from_numpy(idx).to(verts.device)
        self.kept.append(tuple(t.detach().float().index_select(0, sel).clone() for t in (verts, joints_a, joints_b, gt_centred_mm / 1000.0)))

    def tensors(self):
        return tuple(torch.cat([k[i] for k in self.kept]) for i in range(4)) if self.kept else None


# ---- the files ---------------------------------------------------------------------------------------------------------------
def _xyz(v) -> str:
    return '-' if v is None else ' '.join(format(c, '+.2f') for c in v)


def markdown(doc: dict) -> str:
    a, b = doc['j_regressor_initial'], doc['j_regressor_retrained']
    lines = [f'# Regressor report ({doc["source"]})', '',
             f'A, initial: {a["path"]} ({a["sha256_16"]})  ', f'B, retrained: {b["path"]} ({b["sha256_16"]})', '',
             'Displacements B - A of the regressed joints in a frame fixed to the body (x to its left, y up, z forward), in mm.', '',
             f'Pictures: {doc["pictures"]}.  pose_*.png: front | side view of the body, joints of A green, of B blue, ground truth red.  '
             'weights_*.png: the template body with the support vertices of A (green) and B (blue), radius 1.5 + 6 sqrt(weight) px, and '
             'the two regressed joints in pale green and pale blue.', '',
             '| joint | support A | support B | shared | L1 | template shift xyz | mean shift xyz | std xyz | mean abs | pelvis-relative | median | p95 |',
             '|---|---|---|---|---|---|---|---|---|---|---|---|']
    data = doc['data'][ALL]
    for j, r in enumerate(doc['joints']):
        g = lambda key: None if data[key] is None else data[key][j]
        lines.append(f'| {r["joint"]} | {r["support_a"]} | {r["support_b"]} | {r["shared"]} | {r["l1"]:.4f} | {_xyz(r["template_shift_mm"])} | '
                     f'{_xyz(g("mean_mm"))} | {_xyz(g("std_mm"))} | {_f(g("mean_abs_mm"))} | {_f(g("mean_abs_pelvis_relative_mm"))} | '
                     f'{_f(g("median_abs_mm"), ".0f")} | {_f(g("p95_abs_mm"), ".0f")} |')
    lines += ['', f'{data["n"]} poses ({data["n_bad"]} without a body frame or beyond the cap, {doc["data"]["ignored"]} not scored).', '',
              'Mean |B - A| per group and joint, mm:', '', '| group | n | ' + ' | '.join(JOINT_NAMES) + ' |', '|---|---|' + '---|' * NJ]
    for name in doc['groups']:
        r = doc['data']['groups'][name]
        cells = ['-'] * NJ if r['mean_abs_mm'] is None else [format(x, '.1f') for x in r['mean_abs_mm']]
        lines.append(f'| {name} | {r["n"]} | ' + ' | '.join(cells) + ' |')
    lines += ['', 'Heaviest vertices (vertex: weight):', '', '| joint | A | B |', '|---|---|---|']
    for r in doc['joints']:
        fmt = lambda top: ', '.join(f'{t["vertex"]}: {t["weight"]:.3f}' for t in top) or '-'
        lines.append(f'| {r["joint"]} | {fmt(r["top_a"])} | {fmt(r["top_b"])} |')
    return '\n'.join(lines) + '\n'


def write(directory: str, data: dict, joints: List[dict], group_names: Sequence[str], source: str, flags: dict,
          initial: Tuple[Optional[str], Optional[str]], retrained: Tuple[Optional[str], Optional[str]], pictures: str,
          body_model: Optional[str] = None) -> Optional[dict]:
    """DIR/regressor.json and DIR/regressor.md; rank 0 alone writes (the others return None).  data: what finish() returned; joints:
    compare_regressors(); initial / retrained: (path, sha256[:16]); pictures: what was written, or why not"""
    doc = lambda: {'layout_version': LAYOUT_VERSION, 'source': source, 'groups': list(group_names), 'joint_names': list(JOINT_NAMES),
           'frame': 'x = L_Hip - R_Hip, y = up (Neck - Pelvis made orthogonal to x), z = x cross y: forward; from the joints of A',
           'bin_mm': BIN_MM, 'joints': joints, 'data': data, 'flags': flags, 'pictures': pictures, 'body_model': body_model,
           'colours': {'a': list(GREEN), 'b': list(BLUE), 'ground_truth': list(RED), 'joint_a': list(PALE_GREEN), 'joint_b': list(PALE_BLUE)},
           'j_regressor_initial': {'path': initial[0], 'sha256_16': initial[1]},
           'j_regressor_retrained': {'path': retrained[0], 'sha256_16': retrained[1]}}
    return group_table.write(directory, 'regressor', doc, markdown)


def load(directory: str) -> dict:
    return group_table.load(directory, 'regressor', LAYOUT_VERSION)


_OWN_FLAGS = ('regressor_report_depth',)


def flags_doc(flags) -> dict:
    """the flags as the existing output files record them: `regressor_report_depth` changes none of those files, so it is not among them"""
    flags = flags if isinstance(flags, dict) else vars(flags)
    return {k: v for k, v in flags.items() if k not in _OWN_FLAGS}


def check_flags(ns, have_model: bool = False) -> None:
    """what the flags of the report must satisfy, before anything is launched.  have_model: the driver holds a body model of its own
    (the parameter path always does), so the depth section need not resolve one"""
    if getattr(ns, 'regressor_report_depth', False):
        if ns.regressor_report is None:
            raise ValueError('--regressor_report_depth needs --regressor_report DIR (where depth.json / depth.md go)')
        if not have_model and not body_model_available(ns.smpl_dir, ns.synthetic):
            raise ValueError('--regressor_report_depth needs the faces of the body model on every rank: --smpl_dir with SMPL_NEUTRAL.npz / '
                             '.pkl, or --synthetic')
    if ns.regressor_report is None:
        return
    if int(ns.regressor_report_images) < 0:
        raise ValueError(f'--regressor_report_images {ns.regressor_report_images}: 0 or more')
    S = int(ns.regressor_report_size)
    if S % 32 or not 32 <= S <= 256:
        raise ValueError(f'--regressor_report_size {S}: a size the rasteriser takes, a multiple of 32 up to 256')


_MODEL_FILES = ('SMPL_NEUTRAL.npz', 'SMPL_NEUTRAL.pkl', 'smpl_neutral.npz')


def body_model_available(smpl_dir: Optional[str], synthetic: bool) -> bool:
    """whether resolve_body_model would find a body model, without reading one"""
    return bool(synthetic) or bool(smpl_dir and any(os.path.exists(os.path.join(smpl_dir, n)) for n in _MODEL_FILES))


def resolve_body_model(smpl_dir: Optional[str], synthetic: bool) -> Optional[Dict[str, np.ndarray]]:
    """the body model for the pictures of a run that needs none otherwise (`--eval_vertices`): the files of --smpl_dir when they exist,
    the synthetic body under --synthetic, else None (numbers only)"""
    from . import smpl_model
    if smpl_dir and any(os.path.exists(os.path.join(smpl_dir, n)) for n in _MODEL_FILES):
        return smpl_model.load_smpl_model(smpl_dir, allow_synthetic=False)
    if synthetic:
        m = smpl_model.synthetic_smpl()
        m['provenance'] = 'synthetic(seed=1234)'
        return m
    return None


class Run:
    """`--regressor_report` of one evaluation: the table, the kept poses, and at the end the files.  The drivers call add() per
    batch and finish() once; every rank calls both (finish holds the all-reduce), rank 0 writes."""

    def __init__(self, ns, group_names: Sequence[str], device, J_a, J_b, mask, source: str, model_np: Optional[Dict[str, np.ndarray]] = None):
        """model_np: the body model where the driver has one already; the depth section needs its faces on every rank and resolves the
        model itself otherwise"""
        check_flags(ns, have_model=model_np is not None)
        self.ns, self.names, self.device, self.source = ns, list(group_names), torch.device(device), source
        self.J_a, self.J_b = np.asarray(J_a, dtype=np.float32), np.asarray(J_b, dtype=np.float32)
        self.mask = None if mask is None else np.asarray(mask, dtype=np.float32)
        self.table = ShiftReport(self.names, device)
        self.keeper = PoseKeeper(ns.regressor_report_images if _rank() == 0 else 0)
        self.depth, self.depth_model = None, None
        if getattr(ns, 'regressor_report_depth', False):
            self.depth_model = model_np if model_np is not None else resolve_body_model(ns.smpl_dir, ns.synthetic)
            self.depth = DepthReport(self.names, device, self.depth_model['faces'])

    def add(self, verts, joints_a, joints_b, gt_centred_mm, group_ids, scored: Optional[np.ndarray] = None) -> None:
        self.table.add(joints_a, joints_b, group_ids)
        if self.depth is not None:
            if verts is None:
                raise ValueError('--regressor_report_depth: the driver kept no vertices')
            self.depth.add(verts, joints_a, joints_b, gt_centred_mm, group_ids)
        if verts is not None:
            self.keeper.offer(verts, joints_a, joints_b, gt_centred_mm, scored)

    def finish(self, initial, retrained, model_np=None, device_model=None, reduce: bool = True, log=print) -> Optional[dict]:
        """model_np / device_model: the body model for the pictures (device_model None: uploaded here); model_np None: numbers only"""
        data = self.table.finish(reduce=reduce)
        depth_data = self.depth.finish(reduce=reduce) if self.depth is not None else None
        if _rank() != 0:
            return None
        d = self.ns.regressor_report
        os.makedirs(d, exist_ok=True)
        if depth_data is not None:
            write_depth(d, depth_data, template_depth(self.depth_model, self.J_a, self.J_b, self.mask, self.device), self.names, self.source,
                        str(self.depth_model.get('provenance', 'caller-supplied arrays')))
            log(f'regressor report, depth below the skin: {os.path.join(d, "depth.md")}')
        joints = compare_regressors(self.J_a, self.J_b, self.mask, None if model_np is None else model_np['v_template'])
        if model_np is None or model_np.get('faces') is None:
            pictures = 'skipped: no body model'
            log('regressor report: no body model (--smpl_dir does not resolve and --synthetic is not set): numbers only, no pictures')
        else:
            from . import engine as _engine, report as _report
            if device_model is None:
                device_model = _engine.DeviceModel(model_np, self.device)
            pics = Pictures(model_np, device_model, self.ns.regressor_report_size)
            w = pics.weight_pictures(self.J_a, self.J_b, self.mask).cpu().numpy()
            for j in range(NJ):
                _report.write_png(os.path.join(d, f'weights_{j:02d}_{JOINT_NAMES[j]}.png'), w[j])
            kept, n_pose = self.keeper.tensors(), 0
            if kept is not None:
                p = pics.pose_pictures(*kept).cpu().numpy()
                n_pose = p.shape[0]
                for i in range(n_pose):
                    _report.write_png(os.path.join(d, f'pose_{i:05d}.png'), p[i])
            pictures = f'{NJ} weight pictures, {n_pose} pose pictures, {pics.size} x {2 * pics.size}'
        doc = write(d, data, joints, self.names, self.source, eval_protocol.flags_doc(penetration_report.flags_doc(bones_report.flags_doc(flags_doc(ci_report.flags_doc(jargs.recorded(self.ns)))))), initial, retrained, pictures,
                    None if model_np is None else str(model_np.get('provenance', 'caller-supplied arrays')))
        log(f'regressor report: {os.path.join(d, "regressor.md")}')
        return doc
