"""Evaluation report `test_pose_refiner_model()` restated from the reference
(/root/reference/scripts/test.py:33-138, called at /root/reference/main.py:25) on the HIP path.

Per validation batch, under no_grad (reference line numbers):
  :46-53   J_regressor = torch.load('models/retrained_J_Regressor.pt'); J_regressor_initial = J_regressor_h36m.npy;
           mask from the initial regressor
  :59-63   DataLoader(data_set("validation"), batch_size=args.batch_size, shuffle=True, drop_last=True)
  :89-105  SPIN prediction -> rot6d_to_rotmat -> (B,24,3,3)       (here: the batch's own 6-D pose, see optimize.py)
  :107-123 find_joints with the INITIAL regressor -> evaluate -> "before";  with the RETRAINED one -> "after"
  :125-138 print the means of the per-batch MPJPE / PA-MPJPE, 4 decimals, in mm
The SMPL forward runs ONCE per batch for both regressors' joints where the reference runs it twice (the vertices do
not depend on the regressor); `evaluate` is the on-device Procrustes kernel (k_evaluate).
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch

from . import accel_report, batches, bones_report, checkpoint, ci_report, engine as _engine, eval_protocol, eval_report, penetration_report, regressor_report, smpl_model, utils
from . import args as jargs
from .args import args
from .smpl import SMPL


def validation_batches(model_np, J_np, device, with_index: bool = False):
    """the batches the report is computed on (:59-63): the dataset's validation split, shuffled, drop_last=True -- or synthetic
    validation batches with seeds disjoint from the optimiser's.  with_index: dataset batches carry their samples' indices (the same
    batches either way)."""
    if args.data_root:
        return batches.dataset_batches(args.data_root, args.batch_size, args.seed, device, drop_last=True, with_index=with_index)
    return batches.synthetic_batches(model_np, J_np, args.batch_size, args.synthetic_batches, args.seed + 7919)


def _split_paths():
    """the whole split's frame paths, None for synthetic batches and for a split without images.pkl"""
    if not args.data_root:
        return None
    from . import data as jdata
    return jdata.split_image_paths(jdata.split_location('validation', args.data_root))


def _groups():
    """(group names, int32 id per dataset sample or None): from the whole split's frame paths; synthetic batches and a split without
    images.pkl form the single group `all`"""
    paths = _split_paths()
    if paths is None:
        return [eval_report.ALL], None
    return eval_report.assign_groups(paths, args.eval_groups)


def _accel_paths():
    """the whole split's frame paths `--eval_accel` orders the samples by; ValueError naming what is missing"""
    accel_report.check_flags(args._get())
    if not args.data_root:
        raise ValueError('--eval_accel needs --data_root (a dataset whose images.pkl holds the frame paths: they say which samples follow each other)')
    from . import data as jdata
    location = jdata.split_location('validation', args.data_root)
    paths = jdata.split_image_paths(location)
    if paths is None:
        raise ValueError(f'--eval_accel: {os.path.join(location, "images.pkl")} is missing: the frame paths say which samples follow each other')
    return paths


def _ci_units():
    """`--eval_ci`: (unit of every dataset index, number of units) of the whole split for `sequence` units, None for `frame` units (the
    dataset index: the table is sized by the first batch); ValueError naming what is missing"""
    ci_report.check_flags(args._get())
    if args.eval_ci_unit == 'frame':
        return None
    if not args.data_root:
        raise ValueError('--eval_ci --eval_ci_unit sequence needs --data_root (a dataset whose images.pkl holds the frame paths: they say which '
                         'samples share a video sequence), or resample frames: --eval_ci_unit frame')
    from . import data as jdata
    location = jdata.split_location('validation', args.data_root)
    paths = jdata.split_image_paths(location)
    if paths is None:
        raise ci_report.missing_paths_error(os.path.join(location, 'images.pkl'))
    return ci_report.unit_ids('sequence', len(paths), paths)


def _batch_groups(batch, group_ids, B: int, device) -> torch.Tensor:
    """the batch's group ids on the device; samples the batch marks `valid == 0` get -1 (not scored)"""
    gid = torch.zeros(B, dtype=torch.int32)
    if group_ids is not None:
        gid = torch.from_numpy(group_ids[batch['index'].long().numpy()])
    if 'valid' in batch:
        gid = torch.where(batch['valid'].cpu().bool(), gid, torch.full_like(gid, -1))
    return gid.to(device)


def test_pose_refiner_model(retrained_path: Optional[str] = None, log=print) -> Dict[str, float]:
    regressor_report.check_flags(args._get(), have_model=True)      # this path builds its own body model below; refuses before any launch
    accel_paths = _accel_paths() if args.eval_accel else None                                            # refuses before any launch
    ci_units = _ci_units() if args.eval_ci else None                                                     # likewise
    bones_report.check_flags(args._get())                                                                # likewise
    penetration_report.check_flags(args._get())                                                          # likewise: --eval_penetration belongs to --eval_vertices
    eval_protocol.check_flags(args._get())                                                               # likewise: --eval_gt_joints regressed belongs to --eval_vertices
    protocol = eval_protocol.of(args._get())                                                             # of eval.json / ci.json; the printed means stay the 17-joint evaluate
    device = torch.device(args.device)
    torch.cuda.set_device(device)
    smpl = SMPL(args.smpl_dir, batch_size=1, allow_synthetic=args.synthetic or args.smpl_dir == 'SPIN/data/smpl').to(device)   # :40-43
    path = retrained_path or args.eval_j_regressor or args.save_j_regressor or 'models/retrained_J_Regressor.pt'
    J_regressor = checkpoint.load_j_regressor(path).to(device)                                          # :46-47
    J_np = smpl_model.default_h36m_regressor(args.j_regressor_init,
                                             allow_default=args.synthetic or args.j_regressor_init == 'SPIN/data/J_regressor_h36m.npy')
    J_regressor_initial = torch.from_numpy(J_np).float().to(device)                                      # :48-49
    j_reg_mask = utils.find_j_reg_mask(J_regressor_initial)                                              # :51-53

    source = validation_batches(smpl.model_np, J_np, device, with_index=bool(args.eval_report or args.regressor_report or args.eval_accel or args.eval_ci))
    reports, group_ids = None, None
    shift = None
    if args.regressor_report:  # what the retrained regressor did to each joint: one more launch per batch, the vertices of its forward kept
        names, group_ids = _groups()
        depth_model = {'model_np': smpl.model_np} if args.regressor_report_depth else {}      # --regressor_report_depth: the faces are here already
        shift = regressor_report.Run(args._get(), names, device, J_np, J_regressor.cpu().numpy(), j_reg_mask.cpu().numpy(), 'parameters', **depth_model)
    if args.eval_report:       # per group / per joint / PCK next to the four printed means: two more launches per evaluate, no read-back
        names, group_ids = _groups()
        reports = {'before': eval_report.EvalReport(names, device, protocol), 'after': eval_report.EvalReport(names, device, protocol)}
    track = accel_report.JointTrack(len(accel_paths), 2, device) if accel_paths is not None else None
    bones, subject_ids = None, None
    if args.eval_bones:        # the skeleton beside the points: one launch per regressor and one per table, no read-back
        subject_names, subject_ids = bones_report.subjects_of(_split_paths())
        bones = bones_report.BoneReport(names, subject_names, device)
    ci, ci_seen = None, 0      # --eval_ci: the paired bootstrap's unit table, opened at the first batch (frame units: one per sample of the split)

    mpjpe_before, pampjpe_before, mpjpe_after, pampjpe_after = [], [], [], []
    engines: Dict[int, _engine.RefineEngine] = {}
    with torch.no_grad():
        for batch in source:
            B = int(batch['pose6d'].shape[0])
            if B not in engines:
                engines[B] = _engine.RefineEngine(smpl.device_model, B, flags=_engine.FLAG_KEEP_VERTS) if shift is not None else \
                    _engine.RefineEngine(smpl.device_model, B)
            eng = engines[B]
            x6d = batch['pose6d'].to(device).float().contiguous()
            betas = batch['betas'].to(device).float().contiguous()
            gt = utils.move_pelvis(batch['gt_j3d'].to(device).float())                                   # :87
            eng.set_j_regressor(J_regressor_initial, j_reg_mask)
            if shift is not None:
                joints, verts = eng.find_joints_forward(betas, x6d=x6d, return_verts=True)
                joints_initial = joints
            else:
                joints = eng.find_joints_forward(betas, x6d=x6d)                                         # :107-108
            mb, pb = utils.evaluate(joints, gt)                                                         # :110-111
            joints_before = joints
            if reports is not None or shift is not None:
                gid = _batch_groups(batch, group_ids, B, device)
            if reports is not None:
                reports['before'].add(joints, gt, gid)
            eng.set_j_regressor(J_regressor, j_reg_mask)
            joints = eng.find_joints_forward(betas, x6d=x6d)                                             # :116-117
            ma, pa = utils.evaluate(joints, gt)                                                         # :119-120
            mpjpe_before.append(mb); pampjpe_before.append(pb); mpjpe_after.append(ma); pampjpe_after.append(pa)
            if reports is not None:
                reports['after'].add(joints, gt, gid)
            if track is not None:
                track.add(batch['index'], (joints_before, joints), gt, batch.get('valid'))
            if bones is not None:
                sid = _batch_groups(batch, subject_ids, B, device) if subject_ids is not None else None
                bones.add('before', joints_before, gt, gid, sid)
                bones.add('after', joints, gt, gid, sid)
            if args.eval_ci:   # three more launches: both regressors' per-joint errors, then the units; nothing read back
                if ci is None:
                    unit_of_row, n_units = ci_units or ci_report.unit_ids('frame', int(batch.get('n_samples', args.synthetic_batches * B)))
                    ci = ci_report.PairedBootstrap(names, unit_of_row, n_units, device, group_ids, protocol=protocol)
                ci.add(joints_before, joints, gt, gid, batch['index'] if 'index' in batch else torch.arange(ci_seen, ci_seen + B))
                ci_seen += B
            if shift is not None:
                shift.add(verts, joints_initial, joints, gt, gid, None if 'valid' not in batch else batch['valid'].cpu().bool().numpy())
    if not mpjpe_before:
        raise RuntimeError('no validation batch (drop_last=True needs at least --batch_size samples)')
    mean = lambda xs: float(torch.tensor(xs, dtype=torch.float64).mean())
    rep = {'mpjpe_before': mean(mpjpe_before), 'pampjpe_before': mean(pampjpe_before), 'mpjpe_after': mean(mpjpe_after),
           'pampjpe_after': mean(pampjpe_after), 'batches': len(mpjpe_before), 'retrained_j_regressor': path,
           'body_model': smpl.provenance}
    if reports is not None:    # this function runs in ONE process (main.py: rank 0) on whole batches: nothing to reduce
        results = {k: r.finish(reduce=False) for k, r in reports.items()}
        rep['eval_report'] = eval_report.write(args.eval_report, results, names, args.eval_groups if group_ids is not None else 'none', 'parameters',
                                               eval_protocol.flags_doc(penetration_report.flags_doc(bones_report.flags_doc(regressor_report.flags_doc(ci_report.flags_doc(accel_report.flags_doc(jargs.recorded(args._get()))))))), (args.j_regressor_init, eval_report.sha16(args.j_regressor_init, J_np)),
                                               (path, eval_report.sha16(path)), eval_protocol.document(protocol, 'file', eval_report.JOINT_NAMES))
    if track is not None:      # one launch per regressor over the whole split's time order, one read-back
        rep['accel_report'] = accel_report.write(args.eval_report, track.finish(accel_paths, group_ids, names, ('before', 'after'), reduce=False),
                                                 args.eval_groups, 'parameters')
    if bones is not None:      # the one read-back of both regressors' tables
        rep['bones_report'] = bones_report.write(args.eval_report, bones.finish(reduce=False), args.eval_groups if group_ids is not None else 'none',
                                                 'parameters', results)
    if ci is not None:         # the read-back of the unit table, one launch for all replicates, the read-back of their sums
        rep['ci_report'] = ci_report.write(args.eval_report, ci.finish(args.eval_ci_reps, args.seed, args.eval_ci_level, args.eval_ci_unit, reduce=False),
                                           names, args.eval_groups if group_ids is not None else 'none', 'parameters',
                                           eval_protocol.document(protocol, 'file', eval_report.JOINT_NAMES))
    if shift is not None:
        rep['regressor_report'] = shift.finish((args.j_regressor_init, eval_report.sha16(args.j_regressor_init, J_np)),
                                               (path, eval_report.sha16(path)), smpl.model_np, smpl.device_model, reduce=False)
    log('MPJPE')                                                                                         # :125-138
    log(f"{rep['mpjpe_before']:.4f}")
    log('PAMPJPE')
    log(f"{rep['pampjpe_before']:.4f}")
    log('')
    log('after')
    log('MPJPE')
    log(f"{rep['mpjpe_after']:.4f}")
    log('PAMPJPE')
    log(f"{rep['pampjpe_after']:.4f}")
    if track is not None:
        log(accel_report.summary_line(rep['accel_report']))
    if bones is not None:
        log(bones_report.summary_line(rep['bones_report']))
    if ci is not None:
        log(ci_report.summary_line(rep['ci_report']))
    return rep


test_pose_refiner_model.__test__ = False      # not a pytest test: the reference's function name
