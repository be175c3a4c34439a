"""Flag system of the reference (/root/reference/scripts/args.py:1-103) for this path.

The reference evaluates `parser.parse_args()` at import time and exposes a module-level singleton
`args`.  The same 15 flags are kept with identical names, types and defaults; flags added by this
build (synthetic data, SMPL directory, J-step cadence, checkpoint output) never rename existing
ones.  `args` is parsed lazily from sys.argv on first attribute access (unknown flags are
tolerated so the module can be imported under pytest / torchrun).
"""
from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    # ---- the reference's flags (scripts/args.py:5-21), unchanged ----
    parser.add_argument('--name', type=str)
    parser.add_argument('--train_epochs', type=int, default=1)
    parser.add_argument('--opt_steps', type=int, default=40)
    parser.add_argument('--batch_size', type=int, default=256)
    parser.add_argument('--optimization_batch_size', type=int, default=1)
    parser.add_argument('--learning_rate', type=float, default=1e-4)
    parser.add_argument('--opt_lr', type=float, default=1e-2)
    parser.add_argument('--disc_learning_rate', type=float, default=1e-4)
    parser.add_argument('--opt_disc_learning_rate', type=float, default=1e-3)
    parser.add_argument('--translation_lr', type=float, default=1e-6)
    parser.add_argument('--j_reg_lr', type=float, default=1e-2)
    parser.add_argument('--optimization_rate', type=float, default=1e4)
    parser.add_argument('--wandb_log', action='store_true')
    parser.add_argument('--compute_canada', action='store_true')
    parser.add_argument('--device', type=str, default='cuda:0')
    # ---- additions of this build ----
    parser.add_argument('--smpl_dir', type=str, default='SPIN/data/smpl',
                        help='directory with SMPL_NEUTRAL.{pkl,npz} (optimize.py:96-99); synthetic model if absent')
    parser.add_argument('--j_regressor_init', type=str, default='SPIN/data/J_regressor_h36m.npy',
                        help='initial H36M regressor (optimize.py:105-107); shipped checkpoint support if absent')
    parser.add_argument('--synthetic_batches', type=int, default=2,
                        help='number of synthetic outer batches (the Human3.6M loader of scripts/data.py is out of scope)')
    parser.add_argument('--inner_iters', type=int, default=100, help='pose-refinement iterations per batch (optimize.py:220)')
    parser.add_argument('--j_step_every', type=int, default=100,
                        help='inner iterations per J_regressor step (100 = reference cadence: once per outer batch)')
    parser.add_argument('--j_allreduce', type=str, default='support', choices=['support', 'dense'],
                        help='payload of the in-loop J step all-reduce under data parallelism: the regressor\'s support (8 704 B) or the dense (17,6890) gradient')
    parser.add_argument('--all_vertex_tiles', action='store_true',
                        help='run every joint-loss iteration on all 216 vertex tiles (default: only the tiles that hold an entry of the J_regressor\'s support; same results up to summation order)')
    parser.add_argument('--no_pose_disc', action='store_true', help='drop the pose-discriminator term (BASELINE config 2)')
    parser.add_argument('--shape_disc', action='store_true', help='add the shape-discriminator term (optimize.py:244,249-250)')
    parser.add_argument('--reprojection', action='store_true',
                        help='camera pre-fit (optimize.py:187-199) + 2-D joint term (optimize.py:231-233) on synthetic gt_j2d')
    parser.add_argument('--silhouette', action='store_true',
                        help='soft-silhouette term (optimize.py:234-237, x100) against synthetic masks (BASELINE configs[4])')
    parser.add_argument('--image_masks', action='store_true',
                        help='with --data_root and --silhouette: fit the dataset\'s own Mask-RCNN masks (data.py:115-121,130-132; 224 x 224) '
                             'instead of synthetic ones; frames and masks go through the device image pipeline (data.crop_batch)')
    parser.add_argument('--fit_report', type=str, default=None, metavar='DIR',
                        help='with --silhouette: render the mesh before and after the inner loop (optimize.py:204-218,268-274), put the '
                             'silhouette IoU and the 2-D joint error of both into the record and write overlay PNGs (viz(), :28-74) to DIR')
    parser.add_argument('--fit_report_images', type=int, default=8,
                        help='overlay PNG pairs per outer batch and rank (the first poses of the shard)')
    parser.add_argument('--fit_report_mesh', action='store_true',
                        help='with --fit_report: also write b*_p*_{before,after}_mesh.png, the fitted body shaded from the front (over the '
                             'crop under --image_masks, else over black) and from the side (over grey) in one (S, 2S) picture')
    parser.add_argument('--save_refined', type=str, default=None, metavar='DIR',
                        help='keep the refined poses: DIR/refined.npz with per-sample pose (72, axis-angle) / pose6d / shape / cam / '
                             'has_refined and the per-sample errors, rows at their dataset indices, and DIR/meta.json (refined.py)')
    parser.add_argument('--init_refined', type=str, default=None, metavar='DIR',
                        help='with --data_root: samples that a --save_refined table in DIR holds start from its pose6d / shape / cam '
                             'instead of the dataset\'s initial values; a path that ends in .npz reads that file of its directory '
                             '(DIR/refined_smooth.npz: the table --smooth_refined wrote)')
    parser.add_argument('--smooth_refined', type=str, default=None, metavar='DIR',
                        help='with --data_root: filter the --save_refined table of DIR along time, per run of consecutive frames of one '
                             'camera (the frame paths of images.pkl), write DIR/refined_smooth.npz with the jitter before and after and the '
                             'joint error of both, print one line and exit (refined.smooth)')
    parser.add_argument('--fuse_refined', type=str, default=None, metavar='PATH',
                        help='fuse the table --save_refined wrote (DIR, or a named .npz of it such as DIR/refined_smooth.npz) across the camera '
                             'views of each (scene, frame) of the frame paths: write DIR/refined_fused.npz with the fused records, how far each '
                             'view disagreed and the joint error of both, print one line and exit (refined.fuse_views)')
    parser.add_argument('--fuse_max_deg', type=float, default=30.0,
                        help='--fuse_refined: a view further than this from the medoid view of a joint is left out of the mean; 0: the plain mean')
    parser.add_argument('--place_refined', type=str, default=None, metavar='PATH',
                        help='with --data_root: place every refined pose of the table --save_refined wrote (DIR, or a named .npz of it such as '
                             'DIR/refined_fused.npz) in its real camera -- the translation that brings its 17 joints (--eval_j_regressor, else '
                             'the initial regressor) onto the full-frame gt_j2d under the sample\'s intrinsics; write DIR/refined_placed.npz '
                             'with trans / trans_linear / reproj_px / reproj_px_linear / place_status, DIR/place.json and DIR/place.md, '
                             'print one line and exit (refined.place)')
    parser.add_argument('--place_iters', type=int, default=10,
                        help='--place_refined: Levenberg-Marquardt steps on the pixel error behind the linear start, 0 .. 64')
    parser.add_argument('--place_weights', type=str, default=None, metavar='FILE.npy',
                        help='--place_refined: per-joint weights (N,17); a joint takes part when its weight is finite and > 0 (default: ones)')
    parser.add_argument('--visible_refined', type=str, default=None, metavar='PATH',
                        help='with --data_root: what the real camera sees of every placed pose of DIR/refined_placed.npz (PATH: that file or its '
                             'directory; --place_refined writes it) -- per vertex and per regressed joint (--eval_j_regressor, else the initial '
                             'regressor) whether the body itself hides it or it lies outside the window; write DIR/vertex_visibility.npy, '
                             'DIR/refined_visible.npz, DIR/visible.json, DIR/visible.md and DIR/visible_per_vertex.npy, print one line and exit '
                             '(refined.visible)')
    parser.add_argument('--visible_margin_mm', type=float, default=5.0,
                        help='--visible_refined: a face hides a point when it crosses the ray from the camera centre more than this in front of it')
    parser.add_argument('--visible_window', type=str, default='frame', choices=['frame', 'crop'],
                        help='--visible_refined: outside means outside the frame (--visible_frame) or outside the square find_crop cuts from the '
                             'sample\'s bounding box')
    parser.add_argument('--visible_frame', type=int, nargs=2, default=[1000, 1000], metavar=('W', 'H'),
                        help='--visible_refined --visible_window frame: the size of the frame in pixels')
    parser.add_argument('--smooth_sigma', type=float, default=2.0, help='--smooth_refined: standard deviation of the Gaussian, in sampled frames')
    parser.add_argument('--smooth_radius', type=int, default=None,
                        help='--smooth_refined: the window reaches this many frames to either side, 0 .. 16 (default: min(16, ceil(3 sigma)))')
    parser.add_argument('--fit_regressor', type=str, default=None, metavar='OUT',
                        help='with --fit_from: fit the J_regressor on a table of fixed meshes -- Adam steps (--j_reg_lr, minibatches of '
                             '--batch_size) over the support vertices of --j_regressor_init alone, no SMPL forward in the loop -- write '
                             'OUT/retrained_J_Regressor.pt (or --save_j_regressor) and OUT/fit.json, print one line and exit (regressor_fit.py)')
    parser.add_argument('--fit_from', type=str, default=None, metavar='PATH',
                        help='--fit_regressor: a --save_refined directory or a named .npz of it (refined_smooth.npz, refined_fused.npz; '
                             'needs --data_root for the ground truth), or a directory in the --eval_vertices format (no body model is read)')
    parser.add_argument('--fit_epochs', type=int, default=10, help='--fit_regressor: passes over the training rows')
    parser.add_argument('--fit_shuffle', action='store_true', help='--fit_regressor: permute the training rows between epochs (seeded by --seed)')
    parser.add_argument('--fit_holdout', type=float, default=0.1,
                        help='--fit_regressor: fraction F kept out of training and scored beside it: every round(1/F)-th sequence of the '
                             'frame paths in sorted order, without paths the last F of the rows; 0: train on everything')
    parser.add_argument('--fit_solve', action='store_true',
                        help='--fit_regressor: instead of Adam epochs, solve the fit exactly -- with the meshes fixed the loss is a convex '
                             'quadratic in the normalised weights, each row on the simplex over its listed entries; one fp64 pass over the '
                             'table gives its moments (jrr_jfit_moments) and a projected Newton method the minimiser, with the Frank-Wolfe '
                             'gap as the certificate 0 <= loss - optimum <= gap.  Writes OUT/solve.json (not fit.json) and the checkpoint; the '
                             'normalised weights become the raw values (regressor_solve.py)')
    parser.add_argument('--fit_rings', type=int, default=0, metavar='K',
                        help='--fit_solve: let each row\'s support grow over the mesh -- every vertex within K edges of one of its positive '
                             'entries is a candidate (at most 128 per row), which Adam cannot do (relu\'(0) = 0); needs the faces of the '
                             'body model: --smpl_dir or --synthetic')
    parser.add_argument('--fit_solve_tol', type=float, default=1e-6,
                        help='--fit_solve: stop when the Frank-Wolfe gap is at most this fraction of the initial loss')
    parser.add_argument('--fit_solve_iters', type=int, default=1000,
                        help='--fit_solve: most Newton steps; solve.json says `converged: false` when they end the solve')
    parser.add_argument('--fit_solve_loss', type=str, default='mse', choices=['mse', 'mpjpe'],
                        help='--fit_solve: what the solve minimises.  mse: the mean squared joint error the Adam epochs train with.  mpjpe: '
                             'the mean Euclidean distance per joint, the figure every report states -- convex too, solved by reweighted '
                             'fp64 moment passes (jrr_jfit_norm_moments) with the certificate MPJPE - optimum <= gap + delta; solve.json '
                             'gains the key `norm`')
    parser.add_argument('--fit_solve_delta_mm', type=float, default=0.01,
                        help='--fit_solve_loss mpjpe: the smoothing of the norm, sqrt(|r|^2 + delta^2), in mm; finite and > 0')
    parser.add_argument('--fit_grow', type=int, default=None, metavar='R',
                        help='--fit_solve: price EVERY mesh vertex at the solution (jrr_jfit_price: the gradient of the loss with respect to '
                             'a weight on each of the 6890 vertices), report the Frank-Wolfe gap over the whole mesh and grow the support where '
                             'the data want it -- up to R rounds, each adding the vertices with the most negative reduced cost and solving '
                             'again (0: certify only); solve.json gains the key `grow`')
    parser.add_argument('--fit_grow_add', type=int, default=8, metavar='A',
                        help='--fit_grow: most vertices a row adds per round, 1 .. 128')
    parser.add_argument('--eval_report', type=str, default=None, metavar='DIR',
                        help='evaluation report: DIR/eval.json and DIR/eval.md with MPJPE / PA-MPJPE per group and per joint, PCK and AUC, '
                             'initial against retrained regressor (eval_report.py); the printed lines of scripts/test.py:125-138 stay as they are')
    parser.add_argument('--eval_groups', type=str, default='action', choices=['action', 'subject', 'none'],
                        help='groups of the evaluation report, from the frame path (scripts/data.py:301): the component before '
                             'imageSequence without its trailing take number, or the one before that; samples without such a path form '
                             'the single group `all`')
    parser.add_argument('--eval_vertices', type=str, default=None, metavar='DIR',
                        help='with --eval_report and / or --regressor_report: evaluate both regressors on the meshes of DIR (vertices.npy (N,6890,3) float32 m in SMPL '
                             'vertex order, gt_j3d.npy (N,17,3) mm, optional paths.txt or group.npy + group_names.txt) and exit -- what '
                             'scripts/test.py:141-301 does with the vertices of other models; no SMPL model file is read.  The regressors '
                             'are multiplied by find_j_reg_mask of the initial one as at scripts/test.py:108 (the convention of '
                             'test_pose_refiner_model; :206-212 applies no mask -- the reference\'s mask is all ones, so the two agree)')
    parser.add_argument('--eval_protocol', type=str, default='h36m17', choices=['h36m17', 'lsp14', 'lsp14_hips'],
                        help='the protocol of eval.json / eval.md and ci.json / ci.md (eval_protocol.py): h36m17 -- all 17 joints centred on '
                             'joint 0, the reference\'s evaluate; lsp14 -- the 14 LSP joints (the 17 minus Pelvis, Torso and Nose) centred on '
                             'joint 0, Procrustes alignment on the 14 alone: SPIN, METRO; lsp14_hips -- the same 14 centred on the midpoint of '
                             'the hips (joints 1 and 4): VIBE and its descendants.  The four printed means of scripts/test.py:125-138 stay '
                             'the 17-joint evaluate; --eval_accel, --eval_bones and --regressor_report run on the 17 joints as before')
    parser.add_argument('--eval_gt_joints', type=str, default='file', choices=['file', 'regressed'],
                        help='where the ground-truth joints come from: file -- gt_j3d.npy / the dataset; regressed -- with --eval_vertices DIR: '
                             'each regressor applied to DIR/gt_vertices.npy in metres (3DPW-style data: the initial regressor\'s predictions '
                             'are scored against the initial regressor\'s ground-truth joints, the retrained one\'s against its own); '
                             'gt_j3d.npy is then neither needed nor read; not with --eval_accel, --eval_bones or --regressor_report')
    parser.add_argument('--eval_accel', action='store_true',
                        help='with --eval_report DIR (the evaluation, --eval_vertices): also write DIR/accel.json and DIR/accel.md, the '
                             'acceleration error of both regressors\' joints along each video sequence -- per run of consecutive frames of '
                             'one camera, from the frame paths (images.pkl; paths.txt) -- in mm per sampled frame^2 (accel_report.py); with '
                             '--smooth_refined / --fuse_refined: the per-sample accel_err_mm_* arrays of the raw and the processed rows')
    parser.add_argument('--eval_bones', action='store_true',
                        help='with --eval_report DIR (the evaluation, --eval_vertices): also write DIR/bones.json and DIR/bones.md, the bone '
                             'length and direction errors of both regressors\' joints (bones_report.py): per bone the mean length, |length '
                             'difference|, bias and direction error, the MPJPE with the true lengths and with the true directions, per '
                             'subject (from the frame paths) the rigidity of each bone, and the left / right asymmetry')
    parser.add_argument('--eval_pve', action='store_true',
                        help='with --eval_vertices DIR --eval_report OUT: also write OUT/pve.json, OUT/pve.md and OUT/pve_per_vertex.npy, the '
                             'per-vertex error (PVE / MPVPE) and its Procrustes-aligned form of the meshes of DIR/vertices.npy against '
                             'DIR/gt_vertices.npy ((N,6890,3) float32 m), both centred at joint 0 of the initial regressor, per group, per '
                             'pose percentile and per vertex (vertex_report.py); no joint regressor is scored')
    parser.add_argument('--eval_pve_parts', action='store_true',
                        help='with --eval_pve: per-part means as well, a vertex belonging to the SMPL joint with its largest skinning weight; '
                             'needs the body model (--smpl_dir, or the synthetic one under --synthetic)')
    parser.add_argument('--eval_penetration', action='store_true',
                        help='with --eval_vertices DIR --eval_report OUT: also write OUT/penetration.json, OUT/penetration.md, '
                             'OUT/penetration_per_vertex.npy and OUT/penetration.npz, the self-penetration of the meshes of DIR/vertices.npy '
                             '(penetration_report.py): every vertex is pushed under the skin along its normal and asked for the winding '
                             'number of the whole surface -- 1 sound, 2 or more inside another piece of the body, 0 thinner than the push; '
                             'per group the share of penetrating poses, per body part and per vertex the counts, per mesh n_pen / n_thin / '
                             'n_unsure; no joint regressor is scored; needs the body model: --smpl_dir or --synthetic')
    parser.add_argument('--eval_penetration_offset_mm', type=float, default=2.0, metavar='MM',
                        help='--eval_penetration: how far a vertex is pushed under the skin, 0 < MM <= 10')
    parser.add_argument('--eval_ci', action='store_true',
                        help='with --eval_report DIR (the evaluation, --eval_vertices): also write DIR/ci.json and DIR/ci.md, paired bootstrap '
                             'intervals of MPJPE / PA-MPJPE before, after and of their difference, per group (ci_report.py): how sure the '
                             'arrow of the report is; the seed is --seed')
    parser.add_argument('--eval_ci_unit', type=str, default='sequence', choices=['sequence', 'frame'],
                        help='--eval_ci: what is resampled with replacement -- whole video sequences (frames that share a camera directory, '
                             'from the frame paths: images.pkl; paths.txt) or single frames (the dataset index; treats frames as independent)')
    parser.add_argument('--eval_ci_reps', type=int, default=10000, metavar='R', help='--eval_ci: the number of resamples')
    parser.add_argument('--eval_ci_level', type=float, default=0.95, help='--eval_ci: the level of the percentile intervals')
    parser.add_argument('--regressor_report', type=str, default=None, metavar='DIR',
                        help='regressor report: DIR/regressor.json and DIR/regressor.md -- per H36M joint the support of the initial and '
                             'the retrained regressor and how far, in a frame fixed to the body, the retrained one moves the joint on the '
                             'evaluated meshes -- with pose_*.png (the joints of both and the ground truth on the shaded body, front | '
                             'side) and weights_*.png (the support vertices on the template body); works with --eval_vertices as well '
                             '(regressor_report.py)')
    parser.add_argument('--regressor_report_images', type=int, default=8, help='--regressor_report: pose pictures (the first scored poses of rank 0)')
    parser.add_argument('--regressor_report_size', type=int, default=256,
                        help='--regressor_report: height S of the (S, 2S) pictures, a size the rasteriser takes (a multiple of 32 up to 256)')
    parser.add_argument('--regressor_report_depth', action='store_true',
                        help='with --regressor_report DIR: also write DIR/depth.json and DIR/depth.md, the depth of each joint below the skin '
                             'of the evaluated meshes -- the joints of both regressors and the ground truth, per group and joint the mean '
                             'signed depth, the share of poses in which the joint is outside the body (winding number of the surface, no '
                             'face normals), median and 5th percentile; needs the faces of the body model: --smpl_dir or --synthetic')
    parser.add_argument('--camera_iters', type=int, default=1000, help='camera pre-fit Adam steps (optimize.py:190)')
    parser.add_argument('--save_j_regressor', type=str, default=None,
                        help='write the trained regressor in the models/retrained_J_Regressor.pt format')
    parser.add_argument('--seed', type=int, default=0)
    parser.add_argument('--eval_j_regressor', type=str, default=None,
                        help='retrained regressor read by the evaluation report (default: --save_j_regressor, else '
                             'models/retrained_J_Regressor.pt as scripts/test.py:46-47)')
    parser.add_argument('--skip_eval', action='store_true', help='main.py: do not run test_pose_refiner_model() after the optimiser')
    parser.add_argument('--dist_backend', type=str, default=None,
                        help='torch.distributed backend under torchrun (default: nccl = RCCL on GPUs); gloo for debugging')
    parser.add_argument('--single_device', action='store_true',
                        help='debug: every rank uses --device (exercises the N > 1 path on a 1-GPU box; use with --dist_backend gloo)')
    parser.add_argument('--data_root', type=str, default=None,
                        help='directory holding precomputed_{train,val}/ in the reference layout (scripts/data.py:49-86); '
                             'synthetic batches if not given')
    parser.add_argument('--synthetic', action='store_true',
                        help='accept the synthetic body model / regressor when --smpl_dir / --j_regressor_init do not exist '
                             '(otherwise a missing explicit path is an error)')
    return parser


REFERENCE_FLAGS = {
    'name': None, 'train_epochs': 1, 'opt_steps': 40, 'batch_size': 256, 'optimization_batch_size': 1,
    'learning_rate': 1e-4, 'opt_lr': 1e-2, 'disc_learning_rate': 1e-4, 'opt_disc_learning_rate': 1e-3,
    'translation_lr': 1e-6, 'j_reg_lr': 1e-2, 'optimization_rate': 1e4, 'wandb_log': False, 'compute_canada': False,
    'device': 'cuda:0'}


PLACE_FLAGS = ('place_refined', 'place_iters', 'place_weights')


def recorded(ns):
    """the flags (a namespace, or a dict) as the output files of the OTHER commands record them: without the flags of `--place_refined`,
    a command of its own that runs none of the code that records flags -- those files keep the bytes they had before the command existed"""
    if isinstance(ns, dict):
        return {k: v for k, v in ns.items() if k not in PLACE_FLAGS}
    return argparse.Namespace(**{k: v for k, v in vars(ns).items() if k not in PLACE_FLAGS})


def get_args(argv=None) -> argparse.Namespace:
    ns, _ = build_parser().parse_known_args(sys.argv[1:] if argv is None else argv)
    return ns


class _LazyArgs:
    """Module-level singleton with the reference's `from scripts.args import args` ergonomics."""
    _ns = None

    def _get(self):
        if _LazyArgs._ns is None:
            _LazyArgs._ns = get_args()
        return _LazyArgs._ns

    def __getattr__(self, k):
        return getattr(self._get(), k)

    def __setattr__(self, k, v):
        setattr(self._get(), k, v)

    def __repr__(self):
        return repr(self._get())


args = _LazyArgs()
