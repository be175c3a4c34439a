"""Entry point with the reference's shape (/root/reference/main.py:1-29):
    python main.py [flags]            (flags: scripts/args.py names + this build's additions)
    torchrun --nproc-per-node N main.py [flags]   (data parallel, one process per GPU over RCCL)
Runs set_seed(0), optimize_pose_refiner() and then the evaluation report test_pose_refiner_model()
(/root/reference/main.py:21-25).  The reference's two further evaluations (test_pose_refiner_model_VIBE_MEVA,
main.py:26-27) need the external VIBE / MEVA checkouts: the networks are out of scope, what those functions do with the
networks' vertices is `--eval_vertices DIR --eval_report OUT` (eval_report.evaluate_vertices), which runs alone and exits.
`--regressor_report DIR` (regressor_report.py) adds to either evaluation what the retrained regressor did to each joint, with pictures.
`--smooth_refined DIR` (refined.smooth_command) filters a `--save_refined` table along time and exits as well;
`--fuse_refined DIR` (refined.fuse_command) fuses its camera views of each frame and exits;
`--place_refined PATH` (refined.place_command) gives every refined pose its translation in the real camera and exits;
`--visible_refined PATH` (refined.visible_command) says which vertices and joints of the placed poses that camera sees and exits.
`--fit_regressor OUT --fit_from PATH` (regressor_fit.py) fits the regressor on a table of fixed meshes and exits; with `--fit_solve`
(regressor_solve.py) it solves that fit exactly from the table's second moments instead of taking Adam epochs.
`--eval_accel` (accel_report.py) adds the acceleration error along each video sequence to the evaluations and to those two commands.
`--eval_bones` (bones_report.py) adds bone length and direction errors to the evaluations.
`--eval_ci` (ci_report.py) adds paired bootstrap intervals of before, after and their difference to the evaluations.
`--eval_protocol` / `--eval_gt_joints` (eval_protocol.py) score the evaluations as published tables do: 14 joints, hip root, mesh GT."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = 'joint-regressor-refinement_amd'
pkg = importlib.import_module(PKG)
args = importlib.import_module(PKG + '.args').args
optimize = importlib.import_module(PKG + '.optimize')
evaluation = importlib.import_module(PKG + '.test')
utils = importlib.import_module(PKG + '.utils')

if __name__ == '__main__':
    if args.wandb_log:
        try:
            import wandb
            wandb.init(project='human_body_pose_optimization', name=args.name)
        except ImportError:
            print('wandb is not installed; logging to stdout')
    utils.set_seed(0)
    importlib.import_module(PKG + '.regressor_report').check_flags(args._get())   # --regressor_report: refused before anything runs
    importlib.import_module(PKG + '.accel_report').check_flags(args._get())       # --eval_accel: likewise
    importlib.import_module(PKG + '.bones_report').check_flags(args._get())       # --eval_bones: likewise
    importlib.import_module(PKG + '.regressor_fit').check_flags(args._get())      # --fit_regressor: likewise
    importlib.import_module(PKG + '.vertex_report').check_flags(args._get())      # --eval_pve: likewise
    importlib.import_module(PKG + '.ci_report').check_flags(args._get())          # --eval_ci: likewise
    importlib.import_module(PKG + '.penetration_report').check_flags(args._get())  # --eval_penetration: likewise
    importlib.import_module(PKG + '.eval_protocol').check_flags(args._get())      # --eval_protocol / --eval_gt_joints: likewise
    if args.fit_regressor:                                                   # Adam steps of the regressor on fixed meshes; no inner loop
        importlib.import_module(PKG + '.regressor_fit').fit_command()
        sys.exit(0)
    if args.eval_vertices:                                                   # scripts/test.py:141-301 on the meshes of a directory
        importlib.import_module(PKG + '.eval_report').evaluate_vertices()
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.barrier()
            dist.destroy_process_group()
        sys.exit(0)
    if args.smooth_refined:                                                  # a --save_refined table along the time axis; no training
        importlib.import_module(PKG + '.refined').smooth_command()
        sys.exit(0)
    if args.fuse_refined:                                                    # ... across the camera views of each frame; no training
        importlib.import_module(PKG + '.refined').fuse_command()
        sys.exit(0)
    if args.place_refined:                                                   # ... into the real camera of each sample; no training
        importlib.import_module(PKG + '.refined').place_command()
        sys.exit(0)
    if args.visible_refined:                                                 # ... and what that camera sees of it; no training
        importlib.import_module(PKG + '.refined').visible_command()
        sys.exit(0)
    res = optimize.optimize_pose_refiner()                                   # main.py:23
    if args.save_refined and int(os.environ.get('RANK', '0')) == 0:
        print(f'refined poses: {os.path.join(args.save_refined, "refined.npz")}')
    if not args.skip_eval and int(os.environ.get('RANK', '0')) == 0:
        # main.py:25.  The reference reads models/retrained_J_Regressor.pt; when this run did not write a checkpoint
        # (--save_j_regressor unset) and that file is absent, the regressor just trained is evaluated through a
        # temporary checkpoint in the same format.
        path = args.eval_j_regressor or args.save_j_regressor
        if path is None and not os.path.exists('models/retrained_J_Regressor.pt'):
            import tempfile
            path = os.path.join(tempfile.mkdtemp(prefix='jrr_'), 'retrained_J_Regressor.pt')
            importlib.import_module(PKG + '.checkpoint').save_j_regressor(res['J_regressor'], path)
        evaluation.test_pose_refiner_model(path)
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
