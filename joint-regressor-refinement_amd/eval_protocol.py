"""The protocol of the evaluation report (`--eval_protocol`, `--eval_gt_joints`): which joints are scored, where both skeletons are
centred, where the ground-truth joints come from.

The reference's `evaluate` (/root/reference/scripts/utils.py:117-145) scores all 17 regressed joints, centres on joint 0 and takes a
stored (17,3) ground truth in millimetres: `h36m17`, the default -- under it nothing here changes a launch or a byte.  Published
tables do not: they score the 14 LSP joints (the 17 minus Pelvis, Torso and Nose; H36M_TO_J14 of the reference's scripts/constants.py
names the same set), fit the Procrustes alignment on those 14 alone, and centre either on joint 0 (`lsp14`: SPIN, METRO) or on the
midpoint of the two hips, joints 1 and 4 (`lsp14_hips`: VIBE and its descendants).  3DPW-style data has no stored 17-joint ground
truth at all: its ground-truth joints are the regressor applied to the ground-truth mesh (`--eval_gt_joints regressed`), so a retrained
regressor moves BOTH sides of the comparison.

A non-default protocol is one launch per `EvalReport.add` (jrr_evaluate_protocol, include/jrr.h): the masked per-joint errors and
their addition to the JRR_EVAL_ACC_* table.  Everything in this module works without a GPU.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Tuple

NJ = 17
ROOT_JOINT0, ROOT_HIPS = 0, 1          # include/jrr.h: JRR_EVAL_ROOT_*
TARGET_MM, TARGET_M = 0, 1             # JRR_EVAL_TARGET_*
MASK_ALL, MASK_LSP14 = 0x1FFFF, 0x1FD7E      # JRR_EVAL_MASK_*
ROOT_NAMES = {ROOT_JOINT0: 'joint0', ROOT_HIPS: 'hips'}
GT_SOURCES = ('file', 'regressed')
DEFAULT, DEFAULT_GT = 'h36m17', 'file'
_OWN_FLAGS = ('eval_protocol', 'eval_gt_joints')


class Protocol(NamedTuple):
    name: str
    joint_mask: int
    root: int
    joints: Tuple[int, ...]            # the joints of joint_mask, ascending

    @property
    def n_joints(self) -> int:
        return len(self.joints)

    @property
    def is_default(self) -> bool:
        return self.joint_mask == MASK_ALL and self.root == ROOT_JOINT0


def make(name: str, joint_mask: int, root: int) -> Protocol:
    joint_mask = int(joint_mask)
    if joint_mask <= 0 or joint_mask & ~MASK_ALL:
        raise ValueError(f'protocol {name!r}: joint mask {joint_mask:#x}: at least one of the 17 joint bits, none at or above bit 17')
    if root not in ROOT_NAMES:
        raise ValueError(f'protocol {name!r}: root {root!r}: one of {sorted(ROOT_NAMES)}')
    return Protocol(str(name), joint_mask, int(root), tuple(i for i in range(NJ) if joint_mask >> i & 1))


PRESETS = {p.name: p for p in (make('h36m17', MASK_ALL, ROOT_JOINT0),          # the reference's evaluate
                               make('lsp14', MASK_LSP14, ROOT_JOINT0),         # SPIN, METRO
                               make('lsp14_hips', MASK_LSP14, ROOT_HIPS))}     # VIBE and its descendants
H36M17 = PRESETS[DEFAULT]


def get(name: Optional[str]) -> Protocol:
    name = DEFAULT if name is None else name
    if name not in PRESETS:
        raise ValueError(f'--eval_protocol {name!r}: one of {tuple(PRESETS)}')
    return PRESETS[name]


def of(ns) -> Protocol:
    """the protocol of a flags namespace (or dict)"""
    return get((ns.get('eval_protocol') if isinstance(ns, dict) else getattr(ns, 'eval_protocol', None)) or DEFAULT)


def gt_source(ns) -> str:
    return (ns.get('eval_gt_joints') if isinstance(ns, dict) else getattr(ns, 'eval_gt_joints', None)) or DEFAULT_GT


def is_default_run(ns) -> bool:
    return of(ns).is_default and gt_source(ns) == DEFAULT_GT


def check_flags(ns) -> None:
    """the refusals of `--eval_protocol` / `--eval_gt_joints`, each naming the flags, before anything is launched"""
    of(ns)
    src = gt_source(ns)
    if src not in GT_SOURCES:
        raise ValueError(f'--eval_gt_joints {src!r}: one of {GT_SOURCES}')
    if src != 'regressed':
        return
    vdir = getattr(ns, 'eval_vertices', None)
    if not vdir:
        raise ValueError('--eval_gt_joints regressed needs --eval_vertices DIR with gt_vertices.npy: the ground-truth joints are each '
                         'regressor applied to the ground-truth meshes')
    for flag in ('eval_accel', 'eval_bones', 'regressor_report'):
        if getattr(ns, flag, None):
            raise ValueError(f'--eval_gt_joints regressed cannot go with --{flag}: that report needs a stored joint ground truth (gt_j3d.npy; '
                             f'--eval_gt_joints file)')
    p = os.path.join(vdir, 'gt_vertices.npy')
    if not os.path.isfile(p):
        raise FileNotFoundError(f'--eval_gt_joints regressed: {p} is missing: --eval_vertices DIR must hold the ground-truth meshes, '
                                f'(N,6890,3) float32 metres')


def flags_doc(flags) -> dict:
    """the flags as the output files record them: with both flags at their defaults they are not among them, so such a run writes the
    bytes it wrote before the flags existed"""
    flags = flags if isinstance(flags, dict) else vars(flags)
    if is_default_run(flags):
        return {k: v for k, v in flags.items() if k not in _OWN_FLAGS}
    return dict(flags)


def document(protocol: Optional[Protocol], gt: str, joint_names) -> Optional[dict]:
    """the `protocol` entry of eval.json / ci.json; None for the default protocol with stored ground truth (no entry)"""
    protocol = H36M17 if protocol is None else protocol
    if protocol.is_default and gt == DEFAULT_GT:
        return None
    return {'name': protocol.name, 'joints': [joint_names[i] for i in protocol.joints], 'joint_mask': protocol.joint_mask,
            'root': ROOT_NAMES[protocol.root], 'gt_joints': gt}


def headline(entry: Optional[dict]) -> str:
    """what the markdown headers say about a `protocol` entry"""
    if not entry:
        return ''
    root = 'joint 0' if entry['root'] == 'joint0' else 'the midpoint of the hips (joints 1 and 4)'
    gt = 'stored ground-truth joints' if entry['gt_joints'] == 'file' else 'ground-truth joints regressed from the ground-truth meshes by each regressor itself'
    return (f'Protocol `{entry["name"]}`: {len(entry["joints"])} joints ({", ".join(entry["joints"])}), centred on {root}, Procrustes '
            f'alignment on these joints alone; {gt}.')
