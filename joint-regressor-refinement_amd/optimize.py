"""The optimisation driver: `optimize_pose_refiner()` restated from the reference
(/root/reference/scripts/optimize.py:88-337) on the HIP path.

Per outer batch (reference line numbers):
  :132-139  DataLoader over data_set(...)                   -> `--data_root` (precomputed tensors in the reference
            layout, data.py) or seeded synthetic "SPIN-init" batches
  :158-162  batch to device, ground-truth joints pelvis-centred
  :164-185  SPIN initial pose (B,24,6) / betas / camera     -> the dataset's pose / orient / betas tensors stand in for
            the SPIN network's prediction (the network and its checkpoint are absent)
  :187-199  camera pre-fit on the 2-D loss                 -> row f1 (`--reprojection`)
  :234-237  silhouette term                                 -> row f2 (`--silhouette`): synthetic target masks, or with `--image_masks` the
            dataset's own (batch['mask_rcnn'], scripts/data.py:115-132) through the device image pipeline (data.crop_batch)
  :201-202  fresh Adam over [pose, orient, betas, cam], lr 1e-2
  :220-265  100 inner iterations                            -> ONE C-ABI call, jrr_refine_run
  :276-284  pose-discriminator update, Adam(lr=args.opt_disc_learning_rate)
  :286-293  shape-discriminator update
  :300-312  J_regressor step, Adam(lr=args.j_reg_lr)        -> + one RCCL all-reduce under data parallelism
  :314-337  MPJPE / PA-MPJPE before and after the J step, logging (all ten scalars of the reference's record)
  :204-218, :268-274 + viz() :28-74  render before / after the loop -> `--fit_report DIR` (off by default): silhouette IoU and
            2-D joint error of both renders in the record, overlay PNGs of the first poses (report.py); with `--fit_report_mesh` also
            the fitted body itself, shaded, front and side view in one PNG per pose and render (k_vertex_normals, k_mesh_shade)
  (scripts/create_smpl_gt.py, dead in the reference)    -> `--save_refined DIR` (off by default): the refined poses as per-sample
            SMPL records, one k_pose_export launch per outer batch, ONE all-reduce and read-back at the end (refined.py);
            `--init_refined DIR` starts the samples such a table holds from it

Data parallelism (new): one process per GPU, the batch is sharded contiguously, per-pose state is
rank-local, the MSE means are normalised by the GLOBAL batch.  The inner loop has no collective.  The
outer step issues ONE sum-all-reduce over a flat bucket

    [ dJ (17 x 6890) | dD (1 840 153) | dShapeD (171) | log-record sums | loss-history records ]  ~ 7.83 MB

followed by the replicated Adam steps; the bucket's scalar tail is read back ONCE per outer batch (no
`.item()` inside the loop, none per shared-parameter step).  The MPJPE of the regressor AFTER its step
needs the stepped regressor, so those two sums ride in the NEXT batch's bucket (a last 2-float
all-reduce flushes them after the final batch): the record of batch k is logged when batch k+1's bucket
has been read.  A J step inside the inner loop (`--j_step_every` < `--inner_iters`) is
jrr_j_regressor_grad[_support] -> one all-reduce (the regressor's support: 8 704 bytes; dist.JStepExchange) ->
jrr_j_step_apply[_support], with no host synchronisation; in a single process the whole loop including those J
steps is ONE C call (jrr_refine_run_j_steps).
Every rank draws the same global batch (same seed) and keeps rows [lo, hi), so a sharded run
reproduces the single-process run on the same global batch.
"""
from __future__ import annotations

import time
from typing import Dict

import numpy as np
import torch

from . import batches, checkpoint, dist as jdist, engine as _engine, refined as jrefined, report as jreport, smpl_model, utils
from .args import args
from .discriminator import Discriminator, Shape_Discriminator
from .smpl import SMPL


class AdamState:
    """torch.optim.Adam state for one flat parameter tensor, stepped by jrr_adam_step."""

    def __init__(self, param: torch.Tensor, lr: float):
        self.m = torch.zeros_like(param)
        self.v = torch.zeros_like(param)
        self.step = torch.zeros(1, dtype=torch.int32, device=param.device)
        self.lr = lr

    def apply(self, param: torch.Tensor, grad: torch.Tensor):
        self.step += 1
        _engine.adam_step(param, grad, self.m, self.v, self.step, self.lr)


N_J = _engine.NUM_H36M * _engine.NUM_VERTS
N_SCALARS = 10     # joint, pose-discriminated, shape-discriminated, pose-D, shape-D, J error, MPJPE / PA-MPJPE before the
                   # J step (sums over the local poses) and the previous batch's MPJPE / PA-MPJPE after its J step


class SharedBucket:
    """The flat gradient + log bucket of one outer step: one buffer, one all-reduce, one read-back."""

    def __init__(self, device, use_pd: bool, use_sd: bool, hist_records: int):
        def pad(n):                # every section starts 256-byte aligned (the C ABI wants 16-byte aligned pointers)
            return (n + 63) // 64 * 64
        nD = _engine.DISC_PARAMS if use_pd else 0
        nS = _engine.SHAPE_DISC_PARAMS if use_sd else 0
        oD, oS = pad(N_J), pad(N_J) + pad(nD)
        oT = oS + pad(nS)
        self.flat = torch.zeros(oT + N_SCALARS + 5 * hist_records, device=device)
        self.dJ = self.flat[:N_J].view(_engine.NUM_H36M, _engine.NUM_VERTS)
        self.dD = self.flat[oD:oD + nD]
        self.dS = self.flat[oS:oS + nS]
        self.tail = self.flat[oT:]                                  # what is read back: scalars, then the history
        self.scalars = self.tail[:N_SCALARS]
        self.hist = self.tail[N_SCALARS:].view(-1, 5)
        self.nbytes = self.flat.numel() * 4

    def put(self, k: int, per_pose: torch.Tensor):
        self.scalars[k:k + 1].copy_(per_pose.sum().reshape(1))

    def read_back(self):
        """(the scalars, the history records) on the host in float64: the ONE read-back of an outer batch"""
        tail = self.tail.cpu().double().numpy()
        return tail[:N_SCALARS], tail[N_SCALARS:].reshape(-1, 5)


def _check_flags():
    """the flag combinations the driver refuses, before anything is set up"""
    if args.fit_report and not args.silhouette:           # the engine must own a rasteriser and the batch a mask
        raise ValueError('--fit_report needs --silhouette')
    if args.fit_report_mesh and not args.fit_report:      # the shaded views are pictures of the report's two renders
        raise ValueError('--fit_report_mesh needs --fit_report')
    if args.init_refined and not args.data_root:
        raise ValueError('--init_refined needs --data_root (the table is keyed by dataset index)')
    if args.image_masks and not (args.data_root and args.silhouette):
        raise ValueError('--image_masks needs --data_root and --silhouette')


class Run:
    """What lives for the whole run (:88-130): the process's place in the job, the body, the three shared parameter sets with their
    Adam states, the engines and the bucket of the outer step."""

    def __init__(self):
        self.dist = jdist.init(args.dist_backend)
        self.rank, local_rank, self.world = jdist.env_rank_world()
        self.device = torch.device(args.device if (self.world == 1 or args.single_device) else f'cuda:{local_rank}')
        torch.cuda.set_device(self.device)
        utils.set_seed(args.seed)

        smpl = SMPL(args.smpl_dir, batch_size=1, allow_synthetic=args.synthetic or args.smpl_dir == 'SPIN/data/smpl')          # :96-99
        self.J_np = smpl_model.default_h36m_regressor(args.j_regressor_init,
                                                      allow_default=args.synthetic or args.j_regressor_init == 'SPIN/data/J_regressor_h36m.npy')
        # the body goes to the device with the regressor's positive columns as a hint for the library's internal vertex order: the
        # support is stored first, so the joint-loss iterations (FLAG_SUPPORT_TILES below) run a handful of tiles
        tiles_mode = not args.all_vertex_tiles and not args.silhouette
        self.smpl = smpl.to(self.device, hint_vertices=np.nonzero((self.J_np > 0).any(0))[0] if tiles_mode else None)
        self.J_regressor = torch.from_numpy(self.J_np).float().to(self.device).contiguous()   # :105-107
        self.j_reg_mask = utils.find_j_reg_mask(self.J_regressor).contiguous()                # :130

        self.use_pd, self.use_sd = not args.no_pose_disc, bool(args.shape_disc)
        self.disc_flat = Discriminator().flat_parameters().to(self.device).contiguous()       # :112-113 (torch default init)
        self.sdisc_flat = Shape_Discriminator().flat_parameters().to(self.device).contiguous()    # :119-120
        self.disc_opt = AdamState(self.disc_flat, args.opt_disc_learning_rate)                # :116-117
        self.sdisc_opt = AdamState(self.sdisc_flat, args.opt_disc_learning_rate)              # :122-123
        self.J_opt = AdamState(self.J_regressor, args.j_reg_lr)                               # :125-126

        # FLAG_SUPPORT_TILES: iterations whose loss reads the joints only run their skinning kernels on the 32-vertex tiles that hold
        # an entry of the regressor's support (51 of 216 for the shipped checkpoint's structure); the other tiles meet a zero block of
        # the regressor (scripts/utils.py:87-92 multiplies them anyway) and a zero vertex adjoint.  Engaged by eng.j_support_info() in
        # engine_for when the support fits the device lists; with the silhouette term every vertex is needed and every tile runs.
        self.flags = _engine.FLAG_KEEP_VERTS | (_engine.FLAG_POSE_DISC if self.use_pd else 0) | (_engine.FLAG_SHAPE_DISC if self.use_sd else 0) \
            | (_engine.FLAG_SILHOUETTE if args.silhouette else 0) | (0 if args.all_vertex_tiles else _engine.FLAG_SUPPORT_TILES)
        self.engines: Dict = {}
        self.n_hist = (args.inner_iters + 9) // 10                                            # :255 `if i % 10 == 0`
        self.bucket = SharedBucket(self.device, self.use_pd, self.use_sd, self.n_hist)
        self.after_sums = torch.zeros(2, device=self.device)     # MPJPE / PA-MPJPE sums after the J step: next batch's bucket

    def engine_for(self, B_local: int, B_global: int):
        """one engine per shard size (the last batch of a dataset may be ragged: drop_last=False)"""
        if B_local not in self.engines:
            self.engines[B_local] = _engine.RefineEngine(self.smpl.device_model, B_local, batch_norm=B_global, flags=self.flags)
        eng = self.engines[B_local]
        eng.set_batch_norm(B_global)
        eng.set_j_regressor(self.J_regressor, self.j_reg_mask)
        eng.j_support_info()      # one small read-back per outer batch: an engine that knows its regressor's support fits the device
        #                           lists enqueues the support-restricted J-step products only (include/jrr.h, jrr_j_support_info)
        if self.use_pd:
            eng.set_pose_disc(self.disc_flat)
        if self.use_sd:
            eng.set_shape_disc(self.sdisc_flat)
        return eng

    def batches(self, with_index: bool):
        """:132-139; every rank draws the same global batches"""
        if not args.data_root:
            return batches.synthetic_batches(self.smpl.model_np, self.J_np, args.batch_size, args.synthetic_batches, args.seed)
        init_refined = jrefined.load_path(args.init_refined) if args.init_refined else None
        return batches.dataset_batches(args.data_root, args.batch_size, args.seed, self.device, image_masks=bool(args.image_masks),
                                       with_index=with_index, init_refined=init_refined)


class Batch:
    """One outer batch as this rank holds it: the global batch's host tensors `full`, the shard's bounds and engine, and its device
    tensors -- SPIN initial values, the poses / betas / camera being refined with their Adam moments, ground truth, targets."""
    gt_j2d = sil_mask = images = invalid = None           # what the optional terms add (steps 2 and 3)


class RecordLog:
    """The MPJPE of the regressor AFTER its step rides in the NEXT batch's bucket, so the record of batch k is held until batch k+1's
    bucket has been read (or, after the last batch, until a 2-float all-reduce of its own), then completed and logged (:323-337)."""

    def __init__(self, rank: int, log):
        self.rank, self.log = rank, log
        self.history = []
        self.held = None

    def hold(self, rec: dict, B_global: int):
        self.held = (rec, B_global)

    def complete(self, after):
        """`after`: the all-reduced MPJPE / PA-MPJPE sums of the held record's batch with the stepped regressor"""
        if self.held is None:
            return
        rec, B_global = self.held
        self.held = None
        mpjpe_a, pampjpe_a = float(after[0]) * 1000 / B_global, float(after[1]) * 1000 / B_global
        rec['mpjpe'], rec['pampjpe'] = mpjpe_a, pampjpe_a
        rec['mpjpe difference'] = rec.pop('_mpjpe_before') - mpjpe_a
        rec['pampjpe difference'] = rec.pop('_pampjpe_before') - pampjpe_a
        self.history.append(rec)
        if self.rank == 0:
            self.log(rec)                                                                   # wandb.log analogue
            if args.wandb_log:
                try:
                    import wandb
                    wandb.log(rec)
                except ImportError:
                    pass

    def flush(self, after_sums: torch.Tensor):
        """after the last batch: its after-the-J-step sums have no next bucket to ride in"""
        if self.held is not None:
            jdist.all_reduce_sum_(after_sums)
            self.complete(after_sums.cpu().double().numpy())


# ---- the steps of one outer batch, in the order the loop of optimize_pose_refiner calls them -----------------------------------------
def _upload_batch(run: Run, it: int, full, export) -> Batch:
    """step 1 (:158-179): this rank's rows of the batch on the device, ground truth pelvis-centred, the poses at their SPIN values, a
    fresh Adam over [pose, orient, betas, cam] (:201-202)"""
    b = Batch()
    b.t_batch = time.perf_counter()
    b.it, b.full, b.B_global = it, full, int(full['pose6d'].shape[0])
    b.lo, b.hi = jdist.shard_bounds(b.B_global, run.rank, run.world)
    B, device = b.hi - b.lo, run.device
    if B == 0:
        raise RuntimeError(f'batch of {b.B_global} poses cannot be sharded over {run.world} ranks')
    b.eng = run.engine_for(B, b.B_global)
    b.spin_pose = full['pose6d'][b.lo:b.hi].to(device).float().contiguous()                 # :166-168,177-178
    b.spin_betas = full['betas'][b.lo:b.hi].to(device).float().contiguous()
    b.gt_mm = full['gt_j3d'][b.lo:b.hi].to(device).float().contiguous()
    b.gt_j3d = utils.move_pelvis(b.gt_mm).contiguous()                                      # :162
    if export is not None:
        export.upload_index(b, device)
    b.x6d = b.spin_pose.clone()                                                             # :177-179 pose + orient
    b.betas = b.spin_betas.clone()
    b.m = torch.zeros(B, 154, device=device)                                                # :201-202 fresh optimizer
    b.v = torch.zeros(B, 154, device=device)
    b.step = torch.zeros(1, dtype=torch.int32, device=device)
    b.sq = torch.zeros(B, device=device)
    b.cam = full['cam'][b.lo:b.hi].to(device).float().contiguous()                          # :170-172 pred_cam_t
    b.cam_m, b.cam_v = torch.zeros_like(b.cam), torch.zeros_like(b.cam)
    return b


def _fit_camera(b: Batch):
    """step 2 (:170-173,187-199,231-233; row f1): the 2-D target, the camera pre-fit on it, the 2-D term switched on"""
    if 'gt_j2d' in b.full:
        b.gt_j2d = b.full['gt_j2d'][b.lo:b.hi].to(b.cam.device).float().contiguous()
    else:
        b.gt_j2d = _synthetic_gt_j2d(b.eng, b.x6d, b.betas, b.cam, b.full['seed'], b.lo, b.hi, b.B_global)
    b.eng.camera_prefit(b.x6d, b.betas, b.gt_j2d, b.cam, n_steps=args.camera_iters, lr=1e-2)    # :187-199
    b.eng.set_reprojection(b.gt_j2d, b.cam, b.cam_m, b.cam_v)


def _silhouette_target(b: Batch):
    """step 3 (:234-237): the mask the silhouette term fits -- batch['mask_rcnn'] (scripts/data.py:115-132) under `--image_masks`,
    else a synthetic one (row f2)"""
    if args.image_masks:
        b.images = batches.dataset_images(b.full, b.lo, b.hi, b.cam.device, b.eng.sil)
        b.sil_mask = b.images['mask_rcnn'][:, 0].contiguous()
        b.invalid = (~b.images['valid']).sum().float().reshape(1)     # (`valid` is loaded and never used, :159; counted for the record)
        jdist.all_reduce_sum_(b.invalid)
    else:
        b.sil_mask = _synthetic_mask(b.eng, b.x6d, b.betas, b.cam, b.full['seed'], b.lo, b.hi, b.B_global)


def _inner_iterations(run: Run, b: Batch):
    """step 4 (:220-265): the 100 inner iterations; J steps inside the loop only when --j_step_every < --inner_iters"""
    eng, J_opt = b.eng, run.J_opt
    state = (b.x6d, b.betas, b.gt_j3d, b.m, b.v, b.step, 1e-2)
    if args.silhouette:
        eng.set_silhouette(b.sil_mask, b.cam, b.cam_m, b.cam_v)
    b.t0 = time.perf_counter()
    eng.set_loss_history(run.n_hist, 10)                                                    # :255-261 (read back with the bucket)
    n_inloop = (args.inner_iters - 1) // args.j_step_every * args.j_step_every if args.inner_iters > 0 else 0
    if n_inloop and run.dist is None:       # one C call for the iterations AND their J steps (no collective needed)
        eng.refine_run_j_steps(*state, n_inloop, args.j_step_every, run.J_regressor, J_opt.m, J_opt.v, J_opt.step, J_opt.lr,
                               mask=run.j_reg_mask, sqerr=b.sq)
    elif n_inloop:
        # the J step's all-reduce carries the regressor's support only (8.7 KB) when it fits the engine's lists, the dense
        # (17,6890) gradient otherwise or with --j_allreduce dense (asked once per batch: one small read-back)
        xch = jdist.JStepExchange(eng, run.bucket.dJ, compact=args.j_allreduce == 'support')
        for done in range(0, n_inloop, args.j_step_every):
            eng.refine_run(*state, args.j_step_every, sqerr=b.sq, after_j_step=done > 0)
            xch.step(run.J_regressor, J_opt.m, J_opt.v, J_opt.step, J_opt.lr, b.x6d, b.betas, b.gt_j3d, mask=run.j_reg_mask)
    eng.refine_run(*state, args.inner_iters - n_inloop, sqerr=b.sq, after_j_step=n_inloop > 0)


def _loss_terms(run: Run, b: Batch):
    """step 5 (:238-261): the last iteration's loss terms and the loss history into the (zeroed) bucket; the optional terms off again"""
    eng, bucket = b.eng, run.bucket
    b.tiles_run = eng.support_tiles()[1]        # vertex tiles the inner iterations ran (asked while the silhouette term is still set)
    b.sv_on, b.sv_n = eng.support_vertices()      # ... or, per support VERTEX, one launch per iteration (include/jrr.h)
    bucket.flat.zero_()
    bucket.put(0, b.sq)                                                                     # joint_loss (:238-239)
    b.pose_disc_sq, b.shape_disc_sq = eng.refine_aux_losses(run.use_pd, run.use_sd) if args.inner_iters > 0 else (None, None)
    if b.pose_disc_sq is not None:
        bucket.put(1, b.pose_disc_sq)                                                       # :246-247
    if b.shape_disc_sq is not None:
        bucket.put(2, b.shape_disc_sq)                                                      # :249-250
    hist = eng.loss_history()
    if hist is not None and hist.shape[0]:
        bucket.hist[:hist.shape[0]].copy_(hist)
    eng.set_loss_history(0)
    if args.reprojection:
        eng.set_reprojection(None)
    if args.silhouette:
        eng.set_silhouette(None)


def _local_gradients(run: Run, b: Batch, export):
    """step 6 (:276-312): the LOCAL gradients of the three shared-parameter steps, written straight into the bucket, and the joint
    errors of the regressor before its step (:314-315); the previous batch's errors after its step ride along"""
    eng, bucket = b.eng, run.bucket
    if run.use_pd:                                                                          # :276-284
        l0 = eng.pose_disc_backward_params(b.x6d, 0.0, bucket.dD)                           # MSE(D(opt.detach()), 0)
        l1 = eng.pose_disc_backward_params(b.spin_pose, 1.0, bucket.dD)                     # MSE(D(spin), 1)
        bucket.put(3, l0 + l1)
    if run.use_sd:                                                                          # :286-293
        l0 = eng.shape_disc_backward_params(b.betas, 0.0, bucket.dS)
        l1 = eng.shape_disc_backward_params(b.spin_betas, 1.0, bucket.dS)
        bucket.put(4, l0 + l1)
    jsq = torch.zeros(b.hi - b.lo, device=run.device)                                       # :300-312
    joints_before = torch.empty(b.hi - b.lo, 17, 3, device=run.device)
    eng.j_regressor_grad(b.x6d, b.betas, b.gt_j3d, sqerr=jsq, out=bucket.dJ, joints=joints_before)
    bucket.put(5, jsq)
    # :314-315 joints of the old regressor; --save_refined keeps the per-pose output of the same launch
    e_b, epa_b = (export.evaluate_sums if export is not None else utils.evaluate_sums)(joints_before, b.gt_mm)
    bucket.scalars[6:7].copy_(e_b.reshape(1)); bucket.scalars[7:8].copy_(epa_b.reshape(1))
    bucket.scalars[8:10].copy_(run.after_sums)                                              # previous batch, after its J step


def _j_step(run: Run, b: Batch):
    """step 8, first half (:300-312, :317-321): the replicated J step and the joints of the stepped regressor.  The three parameter
    sets are independent; the J step goes first so that the joints after it come from the vertices its forward stored -- uploading
    discriminator weights drops that state."""
    J_opt = run.J_opt
    b.eng.j_step_apply(run.J_regressor, run.bucket.dJ, J_opt.m, J_opt.v, J_opt.step, J_opt.lr, mask=run.j_reg_mask)
    joints_after = b.eng.find_joints_after_j_step(b.betas, b.x6d)         # re-regressed from the J step's vertices
    e_a, epa_a = utils.evaluate_sums(joints_after, b.gt_mm)
    run.after_sums = torch.stack([e_a, epa_a])


def _discriminator_steps(run: Run, b: Batch):
    """step 8, second half (:276-293): the replicated discriminator steps, identical on every rank"""
    if run.use_pd:
        run.disc_opt.apply(run.disc_flat, run.bucket.dD)
        b.eng.set_pose_disc(run.disc_flat)
    if run.use_sd:
        run.sdisc_opt.apply(run.sdisc_flat, run.bucket.dS)
        b.eng.set_shape_disc(run.sdisc_flat)


def _record(run: Run, b: Batch, sc, hist_np, fit) -> dict:
    """step 9 (:314-337): all ten scalars of the reference's record from the all-reduced sums `sc`; the four that need the stepped
    regressor are added when the record is completed (RecordLog)"""
    n = b.B_global
    rec = {'batch': b.it, 'joint_loss': sc[0] / (n * 51),
           'pose_discriminated_loss': sc[1] / (n * 25) if b.pose_disc_sq is not None else None,
           'shape_discriminated_loss': sc[2] / n if b.shape_disc_sq is not None else None,
           'pose_discriminator_loss': sc[3] / (n * 25) if run.use_pd else None,
           'shape_discriminator_loss': sc[4] / n if run.use_sd else None,
           'j_regressor_error': sc[5] / (n * 51),
           '_mpjpe_before': sc[6] * 1000 / n, '_pampjpe_before': sc[7] * 1000 / n,
           'loss_history': [[float(x) for x in row] for row in hist_np],                    # :255-261, every 10th iteration
           'seconds': time.perf_counter() - b.t0,                                           # inner loop + outer step, as the reference times nothing finer
           'seconds_batch': time.perf_counter() - b.t_batch,                                # + H->D copies, camera pre-fit, target set-up
           'vertex_tiles_run': b.tiles_run,   # 216, or the tiles of the regressor's support (FLAG_SUPPORT_TILES engaged)
           'support_vertices_run': b.sv_n if b.sv_on else None,      # the vertices the per-vertex iteration ran on (None: tile kernels)
           'body_model': run.smpl.provenance, 'data': 'dataset' if args.data_root else 'synthetic'}
    if args.silhouette:
        rec['masks'] = 'dataset' if args.image_masks else 'synthetic'
        rec['masks_invalid'] = int(b.invalid.item()) if b.invalid is not None else None
    if fit is not None:
        rec.update(fit.record(b))
    return {k: (float(x) if isinstance(x, np.floating) else x) for k, x in rec.items()}


def optimize_pose_refiner(log=print) -> Dict:
    _check_flags()
    run = Run()
    fit = jreport.FitReport(args.fit_report, args.fit_report_images, mesh=args.fit_report_mesh) if args.fit_report else None
    export = jrefined.RefinedExport(args.save_refined, run.J_np, run.smpl.provenance) if args.save_refined else None
    records = RecordLog(run.rank, log)
    b = None
    for it, full in enumerate(run.batches(with_index=export is not None)):                 # :144-148
        b = None       # the previous batch's tensors go back to the allocator BEFORE this batch's are made (and before its clock starts)
        b = _upload_batch(run, it, full, export)
        if args.reprojection:
            _fit_camera(b)
        if args.silhouette:
            _silhouette_target(b)
        # :204-218.  The render runs a forward of its own on the batch's engine: here every later step starts from the poses again
        if fit is not None:
            fit.before(b)
        _inner_iterations(run, b)
        _loss_terms(run, b)
        _local_gradients(run, b, export)
        jdist.all_reduce_sum_(run.bucket.flat)                                              # step 7: THE collective of the outer step
        _j_step(run, b)
        # :268-274.  A forward of its own again: behind the joints after the J step, the batch's last reader of the engine's forward
        if fit is not None:
            fit.after(b)
        if export is not None:
            export.add(b, fit)
        _discriminator_steps(run, b)
        sc, hist_np = run.bucket.read_back()                                                # the ONE read-back of this batch
        records.complete(sc[8:10])                                                          # the previous batch's record
        records.hold(_record(run, b, sc, hist_np, fit), b.B_global)
    records.flush(run.after_sums)
    if args.save_j_regressor and run.rank == 0:
        checkpoint.save_j_regressor(run.J_regressor, args.save_j_regressor)
    if export is not None:
        export.finish()
    out = {'history': records.history, 'J_regressor': run.J_regressor, 'disc_flat': run.disc_flat, 'sdisc_flat': run.sdisc_flat,
           'x6d': b.x6d if b else None, 'betas': b.betas if b else None, 'cam': b.cam if b else None, 'shard': (b.lo, b.hi) if b else (0, 0)}
    if fit is not None:
        out['fit_report'] = fit.last
    if args.save_refined or args.init_refined:
        out['index'] = b.full['index'][b.lo:b.hi] if args.data_root and b else None         # dataset indices of the last shard
    return out


def _synthetic_gt_j2d(eng, x6d, betas, cam, seed, lo, hi, B_global):
    """2-D targets in the 224-crop pixel frame (scripts/data.py:134-138): the current joints seen through a
    perturbed camera, plus pixel noise (stand-in for the H36M annotations).  The noise is drawn for the GLOBAL
    batch and sliced, so a sharded run sees the same targets as the single-process run."""
    from . import renderer
    g = torch.Generator().manual_seed(seed)
    joints = eng.find_joints_forward(betas, x6d=x6d)
    dcam = (torch.randn(B_global, 3, generator=g) * torch.tensor([0.3, 0.3, 3.0]))[lo:hi]
    noise = (torch.randn(B_global, 17, 2, generator=g) * 2.0)[lo:hi]
    p = renderer.project_points(joints, cam + dcam.to(cam.device))[..., :2]
    return (p + noise.to(cam.device)).contiguous()


def _synthetic_mask(eng, x6d, betas, cam, seed, lo, hi, B_global):
    """Target silhouettes (stand-in for batch['mask_rcnn'], scripts/data.py): the current mesh seen through a
    perturbed camera, binarised."""
    g = torch.Generator().manual_seed(seed + 7)
    _, verts = eng.find_joints_forward(betas, x6d=x6d, return_verts=True)
    dcam = (torch.randn(B_global, 3, generator=g) * torch.tensor([0.2, 0.2, 2.0]))[lo:hi]
    cam_true = (cam + dcam.to(cam.device)).contiguous()
    return (eng.silhouette_forward(verts, cam_true) > 0).float().contiguous()
