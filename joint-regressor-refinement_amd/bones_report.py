"""Bone length and direction errors (`--eval_bones`): the skeleton's column of the evaluation report.

Every other report scores points.  The Human3.6M ground truth is a rigid mocap skeleton -- each bone has one length per subject -- while
the regressed joints are linear functions of a deforming skin: their bone lengths change with the pose and need not match the
subject's, and no pose refinement repairs a wrong bone length.  This report says whether an MPJPE that fell was skeleton proportions
or pose, and whether the new joints form a more or less rigid, more or less symmetric skeleton.

Definition (include/jrr.h, jrr_bone_error): bone b = 1 .. 16 joins joint b to PARENT[b]; per pose, on pelvis-centred joints, the 16
predicted and true lengths, the angle between each pair of bones (atan2 of cross and dot) before and after the Procrustes rotation, and
the per-joint error of two rebuilt skeletons -- the predicted directions with the true lengths (`e_dir`: what is left when the
proportions are right) and the true directions with the predicted lengths (`e_len`: what the proportions alone cost).

`BoneReport` owns ONE int64 device tensor: per prediction set a table by the report's groups and, when the frame paths are known, one
by subject (include/jrr.h, JRR_BONE_ACC_*: rows of 192 words + a 2-word trailer).  `add()` is one jrr_bone_error launch and one or two
jrr_bone_accumulate launches and reads nothing back.  `finish()`: ONE sum all-reduce under a process group (exact: integers of disjoint
shards; through the host for gloo), the one read-back, `derive()` in float64 -- the rigidity from the integer sums in Python integers.
`derive`, `rigidity` and `write` work on CPU tensors, as eval_report's do.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import eval_report, group_table
from .group_table import ALL, arrow as _arrow, fmt as _fmt

LAYOUT_VERSION = 1            # include/jrr.h: JRR_BONE_ACC_LAYOUT_VERSION and the offsets below
ROW, TRAILER = 192, group_table.TRAILER
(COUNT, BAD, SUM_LEN_PRED, SUM_LEN_GT, SUM_ABS_DLEN, SUM_ANG, SUM_ANG_PA, SUM_SQ_PRED, SUM_SQ_GT, SUM_Q_PRED, SUM_Q_GT, SUM_ERR_DIR, SUM_ERR_LEN,
 SUM_ASYM_PRED, SUM_ASYM_GT) = 0, 1, 2, 18, 34, 50, 66, 82, 98, 114, 130, 146, 163, 180, 186
NJ, NB, NP = 17, 16, 6
FIXED = float(1 << 24)        # the sums are in units of 2^-24 m or rad
QUNIT = 65536                 # the q of the squared sums: units of 2^-16 m
PARENT = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)
PAIRS = ((4, 1), (5, 2), (6, 3), (11, 14), (12, 15), (13, 16))
PAIR_NAMES = ('pelvis-hip', 'thigh', 'shin', 'neck-shoulder', 'upper arm', 'forearm')
BONE_NAMES = tuple(f'{eval_report.JOINT_NAMES[PARENT[b]]}-{eval_report.JOINT_NAMES[b]}' for b in range(1, NJ))
NO_SUBJECTS = 'no frame paths: the subjects are unknown, the rigidity of a bone over a subject\'s poses is not reported'


def check_flags(ns) -> None:
    """`--eval_bones` belongs to the evaluation commands and needs `--eval_report DIR`"""
    if getattr(ns, 'eval_bones', False) and not ns.eval_report:
        raise ValueError('--eval_bones needs --eval_report DIR (where bones.json / bones.md go)')


def flags_doc(ns) -> dict:
    """the flags as the existing output files record them: `eval_bones` changes none of those files, so it is not among them"""
    src = ns if isinstance(ns, dict) else vars(ns)
    return {k: v for k, v in src.items() if k != 'eval_bones'}


def subjects_of(paths) -> tuple:
    """(subject names or None, int32 id per sample or None) from a whole split's frame paths (eval_report.assign_groups, kind 'subject')"""
    if paths is None:
        return None, None
    return eval_report.assign_groups(paths, 'subject')


class BoneReport:
    def __init__(self, names: Sequence[str], subject_names: Optional[Sequence[str]], device, set_names: Sequence[str] = ('before', 'after')):
        self.names = [str(g) for g in names]
        self.subject_names = None if subject_names is None else [str(s) for s in subject_names]
        self.set_names = [str(s) for s in set_names]
        for what, n in (('groups', len(self.names)), ('subjects', len(self.subject_names or ['-']))):
            group_table.check_groups(n, what)
        self.device = torch.device(device)
        self.words_g = len(self.names) * ROW + TRAILER
        self.words_s = 0 if self.subject_names is None else len(self.subject_names) * ROW + TRAILER
        self.acc = torch.zeros(len(self.set_names) * (self.words_g + self.words_s), dtype=torch.int64, device=self.device)      # what finish() all-reduces

    def _tables(self, s: int):
        at = s * (self.words_g + self.words_s)
        return self.acc[at:at + self.words_g], (self.acc[at + self.words_g:at + self.words_g + self.words_s] if self.words_s else None)

    def add(self, set_name: str, joints: torch.Tensor, gt_mm: torch.Tensor, gid: Optional[torch.Tensor] = None, sid: Optional[torch.Tensor] = None) -> None:
        """the poses of one prediction set: joints (B,17,3) m, gt (B,17,3) mm, gid / sid (B,) int32 on the same device (gid None: group 0;
        < 0: not scored).  One jrr_bone_error launch, one jrr_bone_accumulate per table; nothing is read back."""
        from . import engine as _engine
        s = self.set_names.index(set_name)
        by_group, by_subject = self._tables(s)
        if (by_subject is None) != (sid is None):
            raise ValueError('BoneReport.add: subject ids go with a report that was opened with subject names, and only with one')
        for t in (gid, sid):
            if t is not None and (t.device != joints.device or t.dtype != torch.int32):
                raise ValueError(f'BoneReport.add: ids must be int32 tensors on {joints.device}, got {t.dtype} on {t.device}')
        vals = _engine.bone_error(joints.detach().float(), gt_mm.detach().float().reshape(-1, NJ, 3))
        _engine.bone_accumulate(vals, gid, len(self.names), by_group)
        if by_subject is not None:
            _engine.bone_accumulate(vals, sid, len(self.subject_names), by_subject)

    def finish(self, reduce: bool = True) -> dict:
        """the ONE all-reduce (reduce=False: this process evaluated everything alone), the one read-back, the derivation"""
        table = group_table.all_reduce(self.acc, reduce)                              # THE integer collective
        host = table.cpu().numpy().reshape(len(self.set_names), self.words_g + self.words_s)      # ... and the one read-back
        sets, subjects = {}, {}
        for s, name in enumerate(self.set_names):
            sets[name] = derive(host[s, :self.words_g], self.names)
            if self.words_s:
                subjects[name] = host[s, self.words_g:]
        out = {'sets': sets, 'set_names': list(self.set_names), 'groups': list(self.names), 'subjects': self.subject_names}
        out['rigidity'] = rigidity(subjects, self.subject_names, self.set_names) if self.words_s else None
        if not self.words_s:
            out['rigidity_note'] = NO_SUBJECTS
        return out


def _mean(xs):
    return None if xs is None else float(np.mean(xs))


def _stats(row: np.ndarray) -> dict:
    n = int(row[COUNT])
    out = {'n': n, 'n_bad': int(row[BAD]), 'raw': [int(x) for x in row]}
    per_bone = (('len_pred_mm', SUM_LEN_PRED, 1000.0), ('len_gt_mm', SUM_LEN_GT, 1000.0), ('abs_dlen_mm', SUM_ABS_DLEN, 1000.0),
                ('ang_deg', SUM_ANG, 180.0 / math.pi), ('ang_pa_deg', SUM_ANG_PA, 180.0 / math.pi))
    keys = [k for k, _, _ in per_bone] + ['bias_mm']
    if n == 0:
        out.update({k: None for k in keys})
        out.update({'mean_' + k: None for k in keys})
        out.update({'err_true_lengths_per_joint_mm': None, 'err_true_directions_per_joint_mm': None, 'mpjpe_true_lengths_mm': None,
                    'mpjpe_true_directions_mm': None, 'asym_pred_mm': None, 'asym_gt_mm': None})
        return out
    for k, s0, unit in per_bone:
        out[k] = [float(s / FIXED / n * unit) for s in row[s0:s0 + NB].astype(np.float64)]
    out['bias_mm'] = [float((int(p) - int(g)) / FIXED / n * 1000.0) for p, g in zip(row[SUM_LEN_PRED:SUM_LEN_PRED + NB], row[SUM_LEN_GT:SUM_LEN_GT + NB])]
    for k in keys:
        out['mean_' + k] = _mean(out[k])
    for k, s0 in (('true_lengths', SUM_ERR_DIR), ('true_directions', SUM_ERR_LEN)):
        sums = row[s0:s0 + NJ].astype(np.float64)
        out[f'err_{k}_per_joint_mm'] = [float(s / FIXED / n * 1000.0) for s in sums]
        out[f'mpjpe_{k}_mm'] = float(sums.sum() / FIXED / (NJ * n) * 1000.0)      # / 17 with the pelvis' zero, as jrr_evaluate divides
    for k, s0 in (('asym_pred_mm', SUM_ASYM_PRED), ('asym_gt_mm', SUM_ASYM_GT)):
        out[k] = [float(s / FIXED / n * 1000.0) for s in row[s0:s0 + NP].astype(np.float64)]
    return out


def derive(table: np.ndarray, names: Sequence[str]) -> dict:
    """the numbers of one prediction set from its int64 table (n_groups * 192 + 2 words), per group and for `all`, in float64: n, n_bad,
    per bone the mean predicted and true length, mean |difference|, bias (mean predicted - mean true) in mm, the mean direction error
    before and after the Procrustes rotation in degrees; the means of those over the 16 bones; the MPJPE of the direction-only skeleton
    (`mpjpe_true_lengths_mm`) and of the length-only one (`mpjpe_true_directions_mm`), sum / 2^24 / (17 n) * 1000; per pair the mean
    |left - right| of the predicted and of the true skeleton.  Raises when a pose carried a group id >= n_groups."""
    return group_table.derive(table, names, ROW, _stats, 'bone table')


def std_mm(n: int, sum_q: int, sum_sq: int) -> Optional[float]:
    """the standard deviation in mm of n lengths from the exact integers sum q and sum q^2, q in 2^-16 m: sqrt(n sum q^2 - (sum q)^2) / n"""
    if n <= 0:
        return None
    var_n2 = int(n) * int(sum_sq) - int(sum_q) ** 2          # Python integers: exact, and never negative (Cauchy-Schwarz on integers)
    return math.sqrt(var_n2) / n / QUNIT * 1000.0


def rigidity(tables: Dict[str, np.ndarray], subject_names: Sequence[str], set_names: Sequence[str]) -> dict:
    """per subject and bone the standard deviation (mm) of the bone's length over the subject's poses, for every prediction set and the
    ground truth (taken from the LAST set's table: the poses it counted), and the mean over subjects and bones.  A rigid skeleton
    gives 0.  tables: set name -> the int64 subject table (n_subjects * 192 + 2 words)."""
    S = len(subject_names)
    per = {}
    for name in set_names:
        per[name], _ = group_table.split(tables[name], S, ROW, 'bone subject table', what='subjects', ident='subject id')
    out = {'per_subject': {}, 'unit': 'mm'}
    for i, subject in enumerate(subject_names):
        entry = {'n': {name: int(per[name][i, COUNT]) for name in set_names}}
        for name in set_names:
            r = per[name][i]
            entry[f'{name}_mm'] = [std_mm(int(r[COUNT]), int(r[SUM_Q_PRED + b]), int(r[SUM_SQ_PRED + b])) for b in range(NB)]
        r = per[set_names[-1]][i]
        entry['gt_mm'] = [std_mm(int(r[COUNT]), int(r[SUM_Q_GT + b]), int(r[SUM_SQ_GT + b])) for b in range(NB)]
        out['per_subject'][subject] = entry
    for key in [f'{name}_mm' for name in set_names] + ['gt_mm']:
        vals = [v for e in out['per_subject'].values() for v in e[key] if v is not None]
        out[f'mean_{key}'] = float(np.mean(vals)) if vals else None
    return out


# ---- the files -------------------------------------------------------------------------------------------------------------
def _at(xs, i):
    return None if xs is None else xs[i]


def markdown(doc: dict) -> str:
    first, last = doc['set_names'][0], doc['set_names'][-1]
    b, a = doc['sets'][first], doc['sets'][last]
    lines = [f'# Bone length and direction errors ({doc["source"]}, groups by {doc["group_kind"]})', '',
             f'`{first}` → `{last}`.  Bone = joint to its parent, on pelvis-centred joints.  `true lengths`: MPJPE of the predicted directions with '
             'the true bone lengths (what is left when the proportions are right); `true directions`: MPJPE of the true directions with the '
             'predicted lengths (what the proportions alone cost).  PA direction: after the Procrustes rotation.', '',
             '| group | n | bad | MPJPE | true lengths | true directions | mean \\|Δ length\\| mm | mean bias mm | direction ° | PA direction ° |',
             '|---|---|---|---|---|---|---|---|---|---|']
    for name in list(doc['groups']) + [ALL]:
        rb = b[ALL] if name == ALL else b['groups'][name]
        ra = a[ALL] if name == ALL else a['groups'][name]
        lines.append(f'| {name} | {ra["n"]} | {ra["n_bad"]} | {_arrow(rb.get("mpjpe_mm"), ra.get("mpjpe_mm"))} | '
                     f'{_arrow(rb["mpjpe_true_lengths_mm"], ra["mpjpe_true_lengths_mm"])} | '
                     f'{_arrow(rb["mpjpe_true_directions_mm"], ra["mpjpe_true_directions_mm"])} | {_arrow(rb["mean_abs_dlen_mm"], ra["mean_abs_dlen_mm"])} | '
                     f'{_arrow(rb["mean_bias_mm"], ra["mean_bias_mm"], "+.2f")} | {_arrow(rb["mean_ang_deg"], ra["mean_ang_deg"])} | '
                     f'{_arrow(rb["mean_ang_pa_deg"], ra["mean_ang_pa_deg"])} |')
    lines += ['', f'Per bone, all groups ({first} → {last}):', '',
              '| bone | true length mm | length mm | \\|Δ length\\| mm | bias mm | direction ° | PA direction ° |', '|---|---|---|---|---|---|---|']
    for i, bn in enumerate(doc['bones']):
        rb, ra = b[ALL], a[ALL]
        lines.append(f'| {bn} | {_fmt(_at(ra["len_gt_mm"], i))} | {_arrow(_at(rb["len_pred_mm"], i), _at(ra["len_pred_mm"], i))} | '
                     f'{_arrow(_at(rb["abs_dlen_mm"], i), _at(ra["abs_dlen_mm"], i))} | {_arrow(_at(rb["bias_mm"], i), _at(ra["bias_mm"], i), "+.2f")} | '
                     f'{_arrow(_at(rb["ang_deg"], i), _at(ra["ang_deg"], i))} | {_arrow(_at(rb["ang_pa_deg"], i), _at(ra["ang_pa_deg"], i))} |')
    lines += ['', 'Asymmetry, all groups: mean |left − right| in mm.', '', '| pair | ' + f'{first} → {last}' + ' | ground truth |', '|---|---|---|']
    for i, pn in enumerate(doc['pairs']):
        lines.append(f'| {pn} | {_arrow(_at(b[ALL]["asym_pred_mm"], i), _at(a[ALL]["asym_pred_mm"], i))} | {_fmt(_at(a[ALL]["asym_gt_mm"], i))} |')
    rig = doc.get('rigidity')
    lines += ['', 'Rigidity: the standard deviation in mm of a bone\'s length over one subject\'s poses (a mocap skeleton gives 0).', '']
    if rig is None:
        lines += [doc.get('rigidity_note', NO_SUBJECTS) + '.']
    else:
        lines += [f'Mean over subjects and bones: {_arrow(rig[f"mean_{first}_mm"], rig[f"mean_{last}_mm"], ".3f")}, ground truth {_fmt(rig["mean_gt_mm"], ".3f")}.', '',
                  '| subject | n | ' + ' | '.join(doc['bones']) + ' |', '|---|---|' + '---|' * NB]
        for subject, e in rig['per_subject'].items():
            cells = [f'{_arrow(_at(e[f"{first}_mm"], i), _at(e[f"{last}_mm"], i))} ({_fmt(_at(e["gt_mm"], i))})' for i in range(NB)]
            lines.append(f'| {subject} | {e["n"][last]} | ' + ' | '.join(cells) + ' |')
        lines += ['', f'Cells: {first} → {last} (ground truth).']
    if a.get('ignored'):
        lines += ['', f'{a["ignored"]} samples were not scored (marked invalid by the dataset).']
    lines += ['', summary_line(doc)]
    return '\n'.join(lines) + '\n'


def summary_line(doc: dict) -> str:
    parts = []
    for name in doc['set_names']:
        r = doc['sets'][name][ALL]
        parts.append(f'{name} |Δ length| {_fmt(r["mean_abs_dlen_mm"])} mm, direction {_fmt(r["mean_ang_deg"])}°, true lengths {_fmt(r["mpjpe_true_lengths_mm"])} mm, '
                     f'true directions {_fmt(r["mpjpe_true_directions_mm"])} mm (n {r["n"]}, bad {r["n_bad"]})')
    rig = doc.get('rigidity')
    tail = '' if rig is None else '  rigidity ' + ' → '.join(_fmt(rig[f'mean_{n}_mm'], '.3f') for n in doc['set_names']) + f' mm (ground truth {_fmt(rig["mean_gt_mm"], ".3f")})'
    return 'bones: ' + '  '.join(parts) + tail


def write(directory: str, result: dict, group_kind: str, source: str, eval_results: Optional[Dict[str, dict]] = None) -> Optional[dict]:
    """DIR/bones.json and DIR/bones.md from what finish() returned; rank 0 alone writes (the others return None).  eval_results: set
    name -> what EvalReport.finish() returned in the same run: each group's MPJPE is put beside the two rebuilt skeletons'."""
    if group_table.rank() != 0:        # before the results are joined below
        return None
    doc = dict(result, layout_version=LAYOUT_VERSION, source=source, group_kind=group_kind, joints=list(eval_report.JOINT_NAMES), bones=list(BONE_NAMES),
               parent=list(PARENT), pairs=list(PAIR_NAMES), pair_bones=[list(p) for p in PAIRS])
    if eval_results is not None:
        for name, res in eval_results.items():
            if name in doc['sets']:
                doc['sets'][name][ALL]['mpjpe_mm'] = res[ALL]['mpjpe_mm']
                for g, r in doc['sets'][name]['groups'].items():
                    r['mpjpe_mm'] = res['groups'][g]['mpjpe_mm']
    return group_table.write(directory, 'bones', doc, markdown)


def load(directory: str) -> dict:
    return group_table.load(directory, 'bones', LAYOUT_VERSION)
