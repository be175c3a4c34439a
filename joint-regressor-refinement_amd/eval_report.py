"""The evaluation report (`--eval_report DIR`, `--eval_vertices DIR`): where the error is.

The reference prints four means (/root/reference/scripts/test.py:125-138).  This module keeps, per group (Human3.6M action or
subject, from the frame's path as /root/reference/scripts/data.py:301 builds it) and for `all`: MPJPE / PA-MPJPE, their 17 per-joint
means, PCK at integer-millimetre thresholds and the AUC of PCK over 0, 5, ..., 150 mm (31 thresholds, the 3DHP convention).

`EvalReport` owns an int64 device table (include/jrr.h, JRR_EVAL_ACC_*: `n_groups` rows of 338 words + a 2-word trailer).  `add()`
is two launches -- jrr_evaluate_joints (the per-joint distances k_evaluate forms before it averages) and jrr_eval_accumulate (integer
atomics) -- and reads nothing back.  `finish()` makes ONE sum-all-reduce under data parallelism (exact: integers of disjoint shards),
then the only read-back, raises on the trailer's status word and derives the numbers in float64.  `finish`, `derive` and `write` work
on a CPU tensor table with a gloo group as well.

`evaluate_vertices()` is `--eval_vertices DIR`: meshes that did not come from this library's SMPL forward
(/root/reference/scripts/test.py:141-301 test_pose_refiner_model_VIBE_MEVA and the METRO block :362-373 do `relu(J) / rowsum`,
`J @ pred_vertices`, `evaluate` on another model's vertices) -- `vertices.npy` (N,6890,3) float32 metres, `gt_j3d.npy` (N,17,3) mm,
optionally `paths.txt` or `group.npy` + `group_names.txt` -- through jrr_regress_joints with both regressors on one read of the
vertices.  No SMPL model file, no engine.  `--eval_pve` adds the per-vertex error of the same meshes against `gt_vertices.npy`
(vertex_report.py): one more launch per chunk, one more all-reduce at the end, and the files above keep their contents.

`--eval_protocol` / `--eval_gt_joints` (eval_protocol.py) choose which joints are scored, where the skeletons are centred and where
the ground-truth joints come from, as published tables do (14 LSP joints, hip root, joints regressed from the ground-truth meshes).
Under the defaults nothing above changes; otherwise `add()` is ONE launch, jrr_evaluate_protocol, and every 17 in a divisor is the
protocol's number of joints.
"""
from __future__ import annotations

import hashlib
import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import args as jargs
from . import dist as jdist
from . import eval_protocol
from . import group_table
from .group_table import ALL, MAX_GROUPS, arrow as _arrow, fmt as _fmt, rank as _rank

LAYOUT_VERSION = 1            # include/jrr.h: JRR_EVAL_ACC_LAYOUT_VERSION and the offsets below
ROW, TRAILER = 338, group_table.TRAILER
COUNT, BAD, SUM, SUM_PA, HIST, HIST_PA, BINS = 0, 1, 2, 19, 36, 187, 151
NJ = 17
FIXED = float(1 << 24)        # the sums are in units of 2^-24 m
PCK_THRESHOLDS_MM = (50, 100, 150)
AUC_THRESHOLDS_MM = tuple(range(0, 151, 5))     # 31 thresholds
JOINT_NAMES = ('Pelvis', 'R_Hip', 'R_Knee', 'R_Ankle', 'L_Hip', 'L_Knee', 'L_Ankle', 'Torso', 'Neck', 'Nose', 'Head',
               'L_Shoulder', 'L_Elbow', 'L_Wrist', 'R_Shoulder', 'R_Elbow', 'R_Wrist')
GROUP_KINDS = ('action', 'subject', 'none')


# ---- groups ----------------------------------------------------------------------------------------------------------------
def group_of(path: Optional[str], kind: str = 'action') -> str:
    """the group of a frame path `.../<subject>/<action>/imageSequence/<camera>/img_%06d.jpg` (scripts/data.py:301): the action is the
    component directly before `imageSequence` with ONE trailing `-N`, `_N`, ` N` or `.N` removed, the subject the component before
    that.  No `imageSequence` component, no path, or kind 'none': the single group `all`."""
    if kind not in GROUP_KINDS:
        raise ValueError(f'group kind {kind!r}: one of {GROUP_KINDS}')
    if kind == 'none' or not path:
        return ALL
    parts = [p for p in re.split(r'[\\/]+', str(path)) if p]
    if 'imageSequence' not in parts:
        return ALL
    at = parts.index('imageSequence')
    want = at - 1 if kind == 'action' else at - 2
    if want < 0:
        return ALL
    name = parts[want]
    if kind == 'action':
        name = re.sub(r'[-_ .]\d+$', '', name, count=1) or name
    return name


def assign_groups(paths: Optional[Sequence[str]], kind: str, n: Optional[int] = None) -> Tuple[List[str], np.ndarray]:
    """(sorted group names, int32 id per sample) of a whole split's paths: every rank computes the same from the same list, so the
    ranks agree without communication.  paths None: the single group `all` for n samples."""
    if paths is None or kind == 'none':
        return [ALL], np.zeros(len(paths) if paths is not None else int(n or 0), dtype=np.int32)
    per = [group_of(p, kind) for p in paths]
    names = sorted(set(per)) or [ALL]
    if len(names) > MAX_GROUPS:
        raise ValueError(f'{len(names)} groups: the accumulator holds at most {MAX_GROUPS}')
    lut = {g: i for i, g in enumerate(names)}
    return names, np.array([lut[g] for g in per], dtype=np.int32)


# ---- the table -------------------------------------------------------------------------------------------------------------
class EvalReport:
    def __init__(self, group_names: Sequence[str], device, protocol: Optional[eval_protocol.Protocol] = None):
        """protocol None or `h36m17`: the reference's evaluate (all 17 joints, centred on joint 0)"""
        self.names = [str(g) for g in group_names]
        self.protocol = eval_protocol.H36M17 if protocol is None else protocol
        group_table.check_groups(len(self.names))
        self.device = torch.device(device)
        self.acc = torch.zeros(len(self.names) * ROW + TRAILER, dtype=torch.int64, device=self.device)

    def add(self, pred_joints: torch.Tensor, gt_j3d_mm: torch.Tensor, group_ids: Optional[torch.Tensor] = None,
            target_unit: int = eval_protocol.TARGET_MM) -> None:
        """pred (B,17,3) m, gt (B,17,3) mm (target_unit TARGET_M: metres), group_ids (B,) int32 on the same device (None: group 0);
        < 0 = do not score.  The default protocol with a millimetre target: two launches (jrr_evaluate_joints, jrr_eval_accumulate);
        any other: ONE launch (jrr_evaluate_protocol) that accumulates.  Nothing read back."""
        from . import engine as _engine
        B = pred_joints.shape[0]
        if group_ids is None:
            group_ids = torch.zeros(B, dtype=torch.int32, device=pred_joints.device)
        if group_ids.device != pred_joints.device or group_ids.dtype != torch.int32:
            raise ValueError(f'EvalReport.add: group_ids must be an int32 tensor on {pred_joints.device}, got {group_ids.dtype} on '
                             f'{group_ids.device}')
        if self.protocol.is_default and target_unit == eval_protocol.TARGET_MM:
            err_j, err_pa_j = _engine.evaluate_joints(pred_joints.detach().float(), gt_j3d_mm.detach().float())
            _engine.eval_accumulate(err_j, err_pa_j, group_ids, len(self.names), self.acc)
            return
        _engine.evaluate_protocol(pred_joints.detach().float(), gt_j3d_mm.detach().float(), self.protocol.joint_mask, self.protocol.root, target_unit,
                                  group_ids, len(self.names), self.acc, rows=False)

    def finish(self, reduce: bool = True) -> dict:
        """the ONE all-reduce (reduce=False: this process evaluated everything alone), the one read-back, the derivation"""
        return derive(group_table.all_reduce(self.acc, reduce).cpu().numpy(), self.names, self.protocol)


def _stats(row: np.ndarray, joints: Optional[Sequence[int]] = None) -> dict:
    """joints: the protocol's joints (None: all 17).  The divisor is their number; an excluded joint has no mean (None)"""
    n, n_bad = int(row[COUNT]), int(row[BAD])
    nj = NJ if joints is None else len(joints)
    out = {'n': n, 'n_bad': n_bad, 'raw': [int(x) for x in row]}
    for key, s0, h0 in (('mpjpe', SUM, HIST), ('pampjpe', SUM_PA, HIST_PA)):
        sums = row[s0:s0 + NJ].astype(np.float64)
        hist = row[h0:h0 + BINS].astype(np.float64)
        if n == 0:
            out.update({f'{key}_mm': None, f'{key}_per_joint_mm': None, f'pck_{key}': None, f'auc_{key}': None})
            continue
        out[f'{key}_mm'] = float(sums.sum() / FIXED / (nj * n) * 1000.0)
        out[f'{key}_per_joint_mm'] = [float(s / FIXED / n * 1000.0) if joints is None or i in joints else None for i, s in enumerate(sums)]
        below = np.concatenate([[0.0], np.cumsum(hist)])                      # below[t] = values < t mm, t = 0 .. 151
        pck = lambda t: float(below[t] / (nj * n))
        out[f'pck_{key}'] = {str(t): pck(t) for t in PCK_THRESHOLDS_MM}
        out[f'auc_{key}'] = float(np.mean([pck(t) for t in AUC_THRESHOLDS_MM]))
    return out


def derive(table: np.ndarray, names: Sequence[str], protocol: Optional[eval_protocol.Protocol] = None) -> dict:
    """the numbers of one regressor's report from the int64 table (n_groups * 338 + 2 words): per group and for `all`
    n, n_bad, MPJPE / PA-MPJPE in mm = sum / 2^24 / (17 n) * 1000 in float64, the 17 per-joint means, PCK@t = (values in bins below t)
    / (17 n), AUC = mean of PCK over t = 0, 5, ..., 150.  Under a protocol of fewer joints every 17 above is the protocol's number of
    joints and the per-joint mean of an excluded joint is None.  Raises when a pose carried a group id >= n_groups."""
    if protocol is None or protocol.joint_mask == eval_protocol.MASK_ALL:
        return group_table.derive(table, names, ROW, _stats, 'evaluation table')
    return group_table.derive(table, names, ROW, lambda row: _stats(row, protocol.joints), 'evaluation table')


# ---- the files -------------------------------------------------------------------------------------------------------------
def sha16(path: Optional[str], fallback: Optional[np.ndarray] = None) -> Optional[str]:
    if path and os.path.isfile(path):
        with open(path, 'rb') as f:
            return hashlib.sha256(f.read()).hexdigest()[:16]
    if fallback is not None:
        return hashlib.sha256(np.ascontiguousarray(fallback).tobytes()).hexdigest()[:16]
    return None


def markdown(doc: dict) -> str:
    reg = doc['regressors']
    first = 'before' if 'before' in reg else sorted(reg)[0]
    last = 'after' if 'after' in reg else sorted(reg)[-1]
    b, a = reg[first], reg[last]
    title = f', protocol {doc["protocol"]["name"]}' if doc.get('protocol') else ''
    lines = [f'# Evaluation report ({doc["source"]}, groups by {doc["group_kind"]}{title})', '',
             f'`{first}`: {doc["j_regressor_initial"]["path"]} ({doc["j_regressor_initial"]["sha256_16"]})  ',
             f'`{last}`: {doc["j_regressor_retrained"]["path"]} ({doc["j_regressor_retrained"]["sha256_16"]})', ''] + \
            ([eval_protocol.headline(doc['protocol']), '',
              'The acceleration, bone and regressor reports (`--eval_accel`, `--eval_bones`, `--regressor_report`) do not know the protocol: '
              'they run as before, on all 17 joints centred on joint 0.', ''] if doc.get('protocol') else []) + \
            [f'Errors in mm, {first} → {last}.  PCK@150 and AUC (PCK over 0, 5, ..., 150 mm) of the unaligned error.', '',
             '| group | n | bad | MPJPE | PA-MPJPE | PCK@150 | AUC |', '|---|---|---|---|---|---|---|']
    for name in list(doc['groups']) + [ALL]:
        rb = b[ALL] if name == ALL else b['groups'][name]
        ra = a[ALL] if name == ALL else a['groups'][name]
        pb = None if rb['pck_mpjpe'] is None else rb['pck_mpjpe']['150']
        pa = None if ra['pck_mpjpe'] is None else ra['pck_mpjpe']['150']
        lines.append(f'| {name} | {ra["n"]} | {ra["n_bad"]} | {_arrow(rb["mpjpe_mm"], ra["mpjpe_mm"])} | '
                     f'{_arrow(rb["pampjpe_mm"], ra["pampjpe_mm"])} | {_arrow(pb, pa, ".4f")} | {_arrow(rb["auc_mpjpe"], ra["auc_mpjpe"], ".4f")} |')
    lines += ['', f'Per joint, all groups ({first} → {last} → difference; negative = the retrained regressor is better):', '',
              '| joint | MPJPE | PA-MPJPE |', '|---|---|---|']
    for i, jn in enumerate(doc['joints']):
        cells = []
        for key in ('mpjpe_per_joint_mm', 'pampjpe_per_joint_mm'):
            vb = None if b[ALL][key] is None else b[ALL][key][i]
            va = None if a[ALL][key] is None else a[ALL][key][i]
            diff = None if vb is None or va is None else va - vb
            cells.append(f'{_arrow(vb, va)} → {_fmt(diff, "+.2f")}')
        lines.append(f'| {jn} | {cells[0]} | {cells[1]} |')
    if a.get('ignored'):
        lines += ['', f'{a["ignored"]} samples were not scored (marked invalid by the dataset).']
    return '\n'.join(lines) + '\n'


def write(directory: str, results: Dict[str, dict], group_names: Sequence[str], group_kind: str, source: str, flags: dict,
          initial: Tuple[Optional[str], Optional[str]], retrained: Tuple[Optional[str], Optional[str]], protocol: Optional[dict] = None) -> Optional[dict]:
    """DIR/eval.json and DIR/eval.md; rank 0 alone writes (the others return None).  `results`: name ('before', 'after') -> what
    finish() returned; initial / retrained: (path, sha256[:16]); protocol: eval_protocol.document(...), None under the default."""
    doc = {'layout_version': LAYOUT_VERSION, 'source': source, 'group_kind': group_kind, 'groups': list(group_names),
           'joints': list(JOINT_NAMES), 'pck_thresholds_mm': list(PCK_THRESHOLDS_MM), 'auc_thresholds_mm': list(AUC_THRESHOLDS_MM),
           'regressors': results, 'flags': flags,
           'j_regressor_initial': {'path': initial[0], 'sha256_16': initial[1]},
           'j_regressor_retrained': {'path': retrained[0], 'sha256_16': retrained[1]}}
    if protocol:
        doc['protocol'] = protocol
    return group_table.write(directory, 'eval', doc, markdown)


def load(directory: str) -> dict:
    return group_table.load(directory, 'eval', LAYOUT_VERSION)


# ---- --eval_vertices -------------------------------------------------------------------------------------------------------
def open_vertices_dir(directory: str, kind: str = 'action', gt_joints: str = 'file'):
    """(vertices memmap (N,6890,3) float32, gt_j3d memmap (N,17,3) float32, group names, int32 ids (N,)) of an --eval_vertices
    directory.  Refuses -- with the file's name -- a wrong shape or dtype, a vertex count other than 6890 and NaN ground truth.
    gt_joints 'regressed' (`--eval_gt_joints regressed`): gt_j3d.npy is neither required nor read, None stands in its place."""
    vp, gp = os.path.join(directory, 'vertices.npy'), os.path.join(directory, 'gt_j3d.npy')
    for p in (vp, gp) if gt_joints != 'regressed' else (vp,):
        if not os.path.isfile(p):
            raise FileNotFoundError(f'--eval_vertices: {p} is missing')
    verts, gt = np.load(vp, mmap_mode='r'), (np.load(gp, mmap_mode='r') if gt_joints != 'regressed' else None)
    if verts.ndim != 3 or verts.shape[2] != 3:
        raise ValueError(f'{vp}: (N,6890,3) expected, got {verts.shape}')
    if verts.shape[1] != 6890:
        raise ValueError(f'{vp}: {verts.shape[1]} vertices per mesh; the regressors are defined on the 6890 SMPL vertices')
    if verts.dtype != np.float32:
        raise ValueError(f'{vp}: float32 expected, got {verts.dtype}')
    N = verts.shape[0]
    if gt is not None and gt.shape != (N, NJ, 3):
        raise ValueError(f'{gp}: ({N},17,3) expected for {N} meshes, got {gt.shape}')
    if gt is not None and gt.dtype not in (np.float32, np.float64):
        raise ValueError(f'{gp}: float32 or float64 expected, got {gt.dtype}')
    if gt is not None and np.isnan(gt).any():
        raise ValueError(f'{gp}: NaN in the ground truth of sample {int(np.argwhere(np.isnan(gt).reshape(N, -1).any(1))[0, 0])}')
    pp, gnp, gip = (os.path.join(directory, f) for f in ('paths.txt', 'group_names.txt', 'group.npy'))
    if kind != 'none' and os.path.isfile(pp):
        with open(pp) as f:
            paths = [line.rstrip('\n') for line in f]
        if len(paths) != N:
            raise ValueError(f'{pp}: {len(paths)} lines for {N} meshes')
        names, ids = assign_groups(paths, kind)
    elif kind != 'none' and os.path.isfile(gip) and os.path.isfile(gnp):
        with open(gnp) as f:
            names = [line.strip() for line in f if line.strip()]
        ids = np.load(gip)
        if ids.shape != (N,) or not np.issubdtype(ids.dtype, np.integer):
            raise ValueError(f'{gip}: ({N},) integers expected, got {ids.dtype} {ids.shape}')
        if ids.size and int(ids.max()) >= len(names):
            raise ValueError(f'{gip}: group id {int(ids.max())} with {len(names)} names in {gnp}')
        ids = ids.astype(np.int32)
    else:
        names, ids = assign_groups(None, 'none', N)
    return verts, gt, names, ids


def read_optional_paths(directory: str, n: int) -> Optional[List[str]]:
    """the frame paths of an --eval_vertices directory (`paths.txt`, one line per mesh), None when the file is absent"""
    p = os.path.join(directory, 'paths.txt')
    if not os.path.isfile(p):
        return None
    with open(p) as f:
        paths = [line.rstrip('\n') for line in f]
    if len(paths) != n:
        raise ValueError(f'{p}: {len(paths)} lines for {n} meshes')
    return paths


def evaluate_vertices(log=print) -> Optional[dict]:
    """`--eval_vertices DIR --eval_report OUT`: rank r takes shard_bounds(N, r, world) of the meshes in chunks of --batch_size
    (pinned uploads), both regressors on one read of the vertices, one all-reduce per report at the end.  `--eval_pve`: the target
    meshes of gt_vertices.npy ride the same loop on a third pinned buffer into vertex_report.VertexReport.  `--eval_penetration`: the
    same device copy of the meshes goes through penetration_report.PenetrationReport, three more launches per chunk."""
    from . import accel_report, bones_report, checkpoint, ci_report, engine as _engine, penetration_report, regressor_report, smpl_model, utils, vertex_report
    from .args import args
    if not args.eval_report and not args.regressor_report:
        raise ValueError('--eval_vertices needs --eval_report or --regressor_report DIR (where eval.json / eval.md, regressor.json / '
                         'regressor.md go)')
    regressor_report.check_flags(args._get())
    accel_report.check_flags(args._get())
    bones_report.check_flags(args._get())
    vertex_report.check_flags(args._get())
    ci_report.check_flags(args._get())
    penetration_report.check_flags(args._get())
    eval_protocol.check_flags(args._get())
    protocol, gt_joints = eval_protocol.of(args._get()), eval_protocol.gt_source(args._get())
    regressed = gt_joints == 'regressed'
    verts, gt, names, ids = open_vertices_dir(args.eval_vertices, args.eval_groups, gt_joints)          # before any launch
    gt_verts = vertex_report.open_gt_vertices(args.eval_vertices, verts.shape[0]) if args.eval_pve or regressed else None
    part_np = None
    if args.eval_pve and args.eval_pve_parts:      # the body model as --regressor_report resolves it; every rank labels the vertices alike
        model_parts = regressor_report.resolve_body_model(args.smpl_dir, args.synthetic)
        if model_parts is None:
            raise ValueError('--eval_pve_parts needs the body model: --smpl_dir with SMPL_NEUTRAL.npz / .pkl, or --synthetic')
        part_np = vertex_report.part_labels(model_parts['lbs_weights'])
    pen_model, pen_sign = None, 0
    if args.eval_penetration:      # the faces and the part labels of the body model; the orientation of the faces from the first finite mesh, on every rank alike
        pen_model = regressor_report.resolve_body_model(args.smpl_dir, args.synthetic)
        pen_sign = penetration_report.orientation(verts, pen_model['faces'])
    accel_paths = accel_report.read_paths(args.eval_vertices, verts.shape[0]) if args.eval_accel else None
    ci_paths = ci_report.read_paths(args.eval_vertices, verts.shape[0]) if args.eval_ci and args.eval_ci_unit == 'sequence' else None
    jdist.init(args.dist_backend)
    rank, local_rank, world = jdist.env_rank_world()
    device = torch.device(args.device if (world == 1 or args.single_device) else f'cuda:{local_rank}')
    torch.cuda.set_device(device)
    if regressed and rank == 0:
        log(f'--eval_gt_joints regressed: the ground-truth joints are each regressor applied to {os.path.join(args.eval_vertices, vertex_report.GT_NAME)}; '
            f'gt_j3d.npy is not read')
    path = args.eval_j_regressor or args.save_j_regressor or 'models/retrained_J_Regressor.pt'
    J_after = checkpoint.load_j_regressor(path).float()
    J_np = smpl_model.default_h36m_regressor(args.j_regressor_init,
                                             allow_default=args.synthetic or args.j_regressor_init == 'SPIN/data/J_regressor_h36m.npy')
    J_before = torch.from_numpy(J_np).float()
    Js = torch.stack([J_before, J_after.cpu()]).to(device)
    table = _engine.JointRegressorTable(Js, utils.find_j_reg_mask(Js[0]))     # the mask of scripts/test.py:51-53,108
    reports = {'before': EvalReport(names, device, protocol), 'after': EvalReport(names, device, protocol)} if args.eval_report else None
    mask_np = utils.find_j_reg_mask(J_before).numpy()
    shift = regressor_report.Run(args._get(), names, device, J_np, J_after.cpu().numpy(), mask_np, 'vertices') if args.regressor_report else None
    N = verts.shape[0]
    track = accel_report.JointTrack(N, 2, device) if accel_paths is not None else None
    bones, subject_ids = None, None
    if args.eval_bones:        # subjects from paths.txt when present; without it the rigidity section says so
        subject_names, subject_ids = bones_report.subjects_of(read_optional_paths(args.eval_vertices, verts.shape[0]))
        bones = bones_report.BoneReport(names, subject_names, device)
    ci = ci_report.PairedBootstrap(names, *ci_report.unit_ids(args.eval_ci_unit, N, ci_paths), device, ids, protocol=protocol) if args.eval_ci else None
    pve = vertex_report.VertexReport(names, device, 6890, part_np, 0 if part_np is None else model_parts['lbs_weights'].shape[1]) if args.eval_pve else None
    root_table = _engine.JointRegressorTable(Js[:1], utils.find_j_reg_mask(Js[0])) if pve is not None else None      # joint 0 of the INITIAL regressor centres both meshes
    pen = penetration_report.PenetrationReport(names, device, pen_model['faces'], N, args.eval_penetration_offset_mm, pen_sign,
                                               vertex_report.part_labels(pen_model['lbs_weights']), pen_model['lbs_weights'].shape[1]) if pen_model is not None else None
    lo, hi = jdist.shard_bounds(N, rank, world)
    bs = max(1, int(args.batch_size))
    stage = [(torch.empty((bs, 6890, 3), dtype=torch.float32).pin_memory(), torch.empty((bs, NJ, 3), dtype=torch.float32).pin_memory(),
              torch.empty((bs,), dtype=torch.int32).pin_memory(), torch.cuda.Event()) for _ in range(2)]
    stage_gt = [torch.empty((bs, 6890, 3), dtype=torch.float32).pin_memory() for _ in range(2)] if gt_verts is not None else None      # --eval_pve, --eval_gt_joints regressed: the third pinned buffer
    used = [False, False]
    with torch.no_grad():
        for k, a in enumerate(range(lo, hi, bs)):
            b = min(a + bs, hi)
            n = b - a
            pv, pg, pi, ev = stage[k % 2]
            if used[k % 2]:
                ev.synchronize()                                              # the upload that last read this buffer is done
            pv.numpy()[:n] = verts[a:b]
            if gt is not None:
                pg.numpy()[:n] = gt[a:b]
            pi.numpy()[:n] = ids[a:b]
            dv, dg, di = (t[:n].to(device, non_blocking=True) for t in (pv, pg, pi))
            if gt_verts is not None:
                stage_gt[k % 2].numpy()[:n] = gt_verts[a:b]
                dq = stage_gt[k % 2][:n].to(device, non_blocking=True)
            ev.record()
            used[k % 2] = True
            joints = table.regress(dv)
            if regressed:      # each regressor's own joints of the ground-truth mesh, in metres: the retrained regressor moves both sides
                gtj = table.regress(dq)
                gts, unit = (gtj[0], gtj[1]), eval_protocol.TARGET_M
            else:
                gtc = utils.move_pelvis(dg)                                   # scripts/test.py:87
                gts, unit = (gtc, gtc), eval_protocol.TARGET_MM
            if reports is not None:
                reports['before'].add(joints[0], gts[0], di, unit)
                reports['after'].add(joints[1], gts[1], di, unit)
            if track is not None:
                track.add(np.arange(a, b), (joints[0], joints[1]), gtc)
            if bones is not None:
                ds = torch.from_numpy(np.where(ids[a:b] >= 0, subject_ids[a:b], -1).astype(np.int32)).to(device) if subject_ids is not None else None
                bones.add('before', joints[0], gtc, di, ds)
                bones.add('after', joints[1], gtc, di, ds)
            if ci is not None:
                ci.add(joints[0], joints[1], gts, di, np.arange(a, b), unit)
            if shift is not None:
                shift.add(dv, joints[0], joints[1], gtc, di, ids[a:b] >= 0)
            if pve is not None:
                pve.add(dv, dq, joints[0][:, 0, :].contiguous(), root_table.regress(dq)[0][:, 0, :].contiguous(), di)
            if pen is not None:
                pen.add(dv, di, a)
    initial, retrained = (args.j_regressor_init, sha16(args.j_regressor_init, J_np)), (path, sha16(path))
    if shift is not None:      # the body model is for the pictures alone: only when --smpl_dir resolves, or --synthetic allows the synthetic one
        model_np = (shift.depth_model or regressor_report.resolve_body_model(args.smpl_dir, args.synthetic)) if rank == 0 else None      # the depth section resolved it already
        shift_doc = shift.finish(initial, retrained, model_np, log=log)
        if reports is None:
            return shift_doc
    results = {k: r.finish() for k, r in reports.items()}
    entry = eval_protocol.document(protocol, gt_joints, JOINT_NAMES)
    doc = write(args.eval_report, results, names, args.eval_groups, 'vertices', eval_protocol.flags_doc(penetration_report.flags_doc(bones_report.flags_doc(regressor_report.flags_doc(ci_report.flags_doc(vertex_report.flags_doc(accel_report.flags_doc(jargs.recorded(args._get())))))))), initial,
                retrained, entry)
    accel_doc = None
    if track is not None:      # every mesh is present and every rank knows it: the float all-reduce, the launches, the integer all-reduce
        accel_doc = accel_report.write(args.eval_report, track.finish(accel_paths, ids, names, ('before', 'after'), present=np.ones(N, dtype=bool)),
                                       args.eval_groups, 'vertices')
    bones_doc = bones_report.write(args.eval_report, bones.finish(), args.eval_groups, 'vertices', results) if bones is not None else None
    ci_doc = ci_report.write(args.eval_report, ci.finish(args.eval_ci_reps, args.seed, args.eval_ci_level, args.eval_ci_unit), names, args.eval_groups,
                             'vertices', entry) if ci is not None else None
    pve_doc = vertex_report.write(args.eval_report, pve.finish(), names, args.eval_groups, 'vertices', initial) if pve is not None else None
    pen_doc = penetration_report.write(args.eval_report, pen.finish(), names, args.eval_groups, 'vertices', args.eval_penetration_offset_mm, pen_sign) if pen is not None else None
    if rank == 0:
        for k in ('before', 'after'):
            r = results[k][ALL]
            log(f'{k}: n {r["n"]} (bad {r["n_bad"]})  MPJPE {_fmt(r["mpjpe_mm"], ".4f")}  PAMPJPE {_fmt(r["pampjpe_mm"], ".4f")}')
        if accel_doc is not None:
            log(accel_report.summary_line(accel_doc))
        if bones_doc is not None:
            log(bones_report.summary_line(bones_doc))
        if pve_doc is not None:
            log(vertex_report.summary_line(pve_doc))
        if ci_doc is not None:
            log(ci_report.summary_line(ci_doc))
        if pen_doc is not None:
            log(penetration_report.summary_line(pen_doc))
        log(f'evaluation report: {os.path.join(args.eval_report, "eval.md")}')
    return doc
