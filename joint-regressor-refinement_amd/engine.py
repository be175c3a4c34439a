"""Thin Python wrappers over the C ABI: device model, per-batch engine, free operator functions.

All tensors are torch CUDA (ROCm) float32 tensors; PyTorch owns every buffer including the
engine workspace, and kernels are enqueued on torch's current stream.
"""
from __future__ import annotations

import ctypes
import functools
from ctypes import byref, c_int32, c_void_p
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

FLAG_POSE_DISC = 1
FLAG_SHAPE_DISC = 2
FLAG_KEEP_VERTS = 4
FLAG_FOLDED = 8
FLAG_SILHOUETTE = 16
FLAG_NO_MODEL = 32
FLAG_SIL_256 = 64      # with FLAG_SILHOUETTE: 256 x 256 silhouettes (the reference constructor's default) instead of 224 x 224
def FLAG_SIL_SIZE(size: int) -> int:
    """with FLAG_SILHOUETTE: an explicit silhouette size, any multiple of 32 up to 256 (include/jrr.h JRR_FLAG_SIL_SIZE)"""
    if size % 32 or not 32 <= size <= 256:
        raise ValueError(f'silhouette size {size}: a multiple of 32 up to 256')
    return (size // 32) << 16


FLAG_SUPPORT_TILES = 128      # joint-loss iterations on the tiles of the regressor's support only (see include/jrr.h)
FLAG_BLEND_BF16X3 = 256       # SIDE MODE, not the reference's arithmetic: split-bf16 blend adjoint (see include/jrr.h); never the default
SIL = 224

NUM_VERTS, NUM_JOINTS, NUM_H36M, NUM_BETAS = 6890, 24, 17, 10
DISC_PARAMS = 1840153
SHAPE_DISC_PARAMS = 171

DISC_KEYS = (['conv_operations.0.weight', 'conv_operations.0.bias', 'conv_operations.2.weight', 'conv_operations.2.bias']
             + [k for i in range(24) for k in (f'linears.{i}.weight', f'linears.{i}.bias')]
             + ['linear_operations.0.weight', 'linear_operations.0.bias', 'linear_operations.2.weight',
                'linear_operations.2.bias', 'linear_operations.4.weight', 'linear_operations.4.bias'])
SHAPE_DISC_KEYS = ['shape_operations.0.weight', 'shape_operations.0.bias', 'shape_operations.2.weight',
                   'shape_operations.2.bias', 'shape_operations.4.weight', 'shape_operations.4.bias']


def flatten_state_dict(sd: Dict[str, torch.Tensor], keys) -> torch.Tensor:
    """state_dict -> the flat parameter vector the C ABI expects (state_dict order)."""
    return torch.cat([sd[k].detach().reshape(-1).float() for k in keys])


def unflatten_state_dict(flat: torch.Tensor, like: Dict[str, torch.Tensor], keys) -> Dict[str, torch.Tensor]:
    out, off = {}, 0
    for k in keys:
        n = like[k].numel()
        out[k] = flat[off:off + n].view_as(like[k])
        off += n
    return out


def _f32c(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


class DeviceModel:
    """SMPL constants uploaded in the kernels' tile-major layouts (jrr_model_create)."""

    def __init__(self, model: Dict[str, np.ndarray], device='cuda:0', hint_vertices=None):
        """hint_vertices (optional): file indices of the vertices the H36M regressor reads (its positive columns); the library stores
        them first internally, so that the iterations of FLAG_SUPPORT_TILES run ceil(n / 32) tiles (jrr_model_create_hinted)"""
        self.lib = _lib.load()
        self.device = torch.device(device)
        vt, sd, pd = _f32c(model['v_template']), _f32c(model['shapedirs']), _f32c(model['posedirs'])
        jr, w = _f32c(model['J_regressor']), _f32c(model['lbs_weights'])
        par = np.ascontiguousarray(np.asarray(model['parents'], dtype=np.int32))
        assert vt.shape == (NUM_VERTS, 3) and sd.shape == (NUM_VERTS, 3, NUM_BETAS) and pd.shape == (207, NUM_VERTS * 3)
        assert jr.shape == (NUM_JOINTS, NUM_VERTS) and w.shape == (NUM_VERTS, NUM_JOINTS) and par.shape == (NUM_JOINTS,)
        self.faces = model.get('faces')
        h = c_void_p()
        # the model's device memory is a torch buffer like every other buffer of the path (jrr_model_create_in)
        nbytes = int(self.lib.jrr_model_bytes())
        self.buffer = torch.zeros(nbytes + 256, dtype=torch.uint8, device=self.device)
        base = (self.buffer.data_ptr() + 255) // 256 * 256
        with torch.cuda.device(self.device):
            if hint_vertices is not None and len(hint_vertices):
                hv = np.ascontiguousarray(np.asarray(hint_vertices, dtype=np.int32).ravel())
                check(self.lib.jrr_model_create_hinted(vt.ctypes.data, sd.ctypes.data, pd.ctypes.data, jr.ctypes.data, w.ctypes.data,
                                                       par.ctypes.data, hv.ctypes.data, int(hv.size), c_void_p(base), nbytes, byref(h)),
                      'jrr_model_create_hinted')
            else:
                check(self.lib.jrr_model_create_in(vt.ctypes.data, sd.ctypes.data, pd.ctypes.data, jr.ctypes.data,
                                                   w.ctypes.data, par.ctypes.data, c_void_p(base), nbytes, byref(h)), 'jrr_model_create_in')
        self.handle = h
        info = (c_int32 * 30)()
        check(self.lib.jrr_model_info(self.handle, info, 30), 'jrr_model_info')
        # what the LBS kernels run for this body: joint slots per tile and pass (0: dense kernels), tiles that need a second
        # pass, the most joints of any tile, whether the library re-ordered the vertices internally, tiles by joint count
        self.info = {'joint_slots': int(info[0]), 'wide_tiles': int(info[1]), 'most_joints_per_tile': int(info[2]),
                     'internal_vertex_order': bool(info[3]), 'tile_joint_histogram': [int(x) for x in info[4:29]],
                     'hinted_vertices_stored_first': int(info[29])}
        if self.faces is not None:
            f = np.ascontiguousarray(np.asarray(self.faces, dtype=np.int32))
            check(self.lib.jrr_model_set_faces(self.handle, f.ctypes.data, int(f.shape[0])), 'jrr_model_set_faces')

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                self.lib.jrr_model_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def overwrites_forward_state(method):
    """Marks a RefineEngine wrapper whose call overwrites what the adjoint entry points read of the MOST RECENT forward
    (RefineEngine.generation): the counter is bumped before the call, so a call that raises has bumped it too."""
    @functools.wraps(method)
    def wrapper(self, *args, **kwargs):
        self.generation += 1
        return method(self, *args, **kwargs)
    wrapper.overwrites_forward_state = True
    return wrapper


class RefineEngine:
    """Per-batch plan over a caller-owned (torch) workspace: jrr_engine_*."""

    def __init__(self, model: Optional[DeviceModel], batch: int, batch_norm: Optional[int] = None, flags: int = 0,
                 device=None):
        """`model` may be None for an engine that serves the discriminators only (flags within POSE_DISC | SHAPE_DISC)"""
        self.lib = model.lib if model is not None else _lib.load()
        self.model = model
        self.device = model.device if model is not None else torch.device(device if device is not None else 'cuda:0')
        self.batch = int(batch)
        self.batch_norm = int(batch_norm or batch)
        self.flags = int(flags) | (FLAG_NO_MODEL if model is None else 0)   # no SMPL workspace for a discriminator-only engine
        self.sil = 32 * ((self.flags >> 16) & 15) or (256 if (self.flags & FLAG_SIL_256) else SIL)      # silhouette image size of this engine
        # Forward-generation counter: the adjoint entry points read the engine's internal state of the MOST RECENT
        # forward (include/jrr.h: "must follow it"), while autograd defers backward.  Every call that overwrites that
        # state bumps the counter (@overwrites_forward_state); the autograd wrappers compare it with the value saved at forward time and re-run
        # the forward from their saved inputs when it has moved (utils._FindJointsFn, smpl._SMPLVerticesFn,
        # discriminator._PoseDiscFn).
        self.generation = 0
        nbytes = self.lib.jrr_engine_workspace_bytes(self.batch, self.flags)
        # zero-filled: padded rows/columns of several sections are read by the GEMM kernels
        self.workspace = torch.zeros(nbytes + 256, dtype=torch.uint8, device=self.device)
        base = (self.workspace.data_ptr() + 255) // 256 * 256
        h = c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.jrr_engine_create(model.handle if model is not None else None, self.batch, int(batch_norm or batch), c_void_p(base), nbytes,
                                             self.flags, byref(h)), 'jrr_engine_create')
        self.handle = h
        info = (c_int32 * 9)()
        self.lib.jrr_engine_info(self.handle, info, 9)
        self.info = dict(zip(['B', 'BP', 'batch_norm', 'nvc', 'nvcb', 'nsplit', 'nsplitJ', 'flags', 'joint_sparse'], list(info)))

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                self.lib.jrr_engine_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # -- helpers ---------------------------------------------------------------------------
    def _s(self):
        return stream_ptr(self.device)

    def _chk(self, t, shape, name):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape), \
            f'{name}: expected contiguous float32 cuda tensor of shape {tuple(shape)}, got {tuple(t.shape)} {t.dtype}'
        return t

    # -- configuration ---------------------------------------------------------------------
    def set_batch_norm(self, n: int):
        check(self.lib.jrr_engine_set_batch_norm(self.handle, int(n)), 'set_batch_norm')
        self.batch_norm = int(n)
        self.info['batch_norm'] = int(n)

    def set_folded(self, enabled: bool):
        """refine_run through the folded regressor tables (engine must have FLAG_FOLDED)"""
        check(self.lib.jrr_engine_set_folded(self.handle, int(bool(enabled)), self._s()), 'set_folded')

    @overwrites_forward_state
    def set_j_regressor(self, J: torch.Tensor, mask: Optional[torch.Tensor] = None):
        J = J.detach().to(self.device, torch.float32).contiguous()      # any stride / device tag
        self._chk(J, (NUM_H36M, NUM_VERTS), 'J_regressor')
        if mask is not None:
            mask = self._chk(mask.detach().to(self.device, torch.float32).contiguous(), (NUM_H36M, NUM_VERTS), 'mask')
        check(self.lib.jrr_engine_set_j_regressor(self.handle, ptr(J), ptr(mask), self._s()), 'set_j_regressor')

    @overwrites_forward_state
    def set_pose_disc(self, flat: torch.Tensor):
        flat = self._chk(flat.detach().to(self.device, torch.float32).contiguous(), (DISC_PARAMS,), 'disc params')
        check(self.lib.jrr_engine_set_pose_disc(self.handle, ptr(flat), self._s()), 'set_pose_disc')

    def set_shape_disc(self, flat: torch.Tensor):
        # no generation bump: the upload overwrites the parameter block Ps alone, and no shape-D operator keeps forward state
        flat = self._chk(flat.detach().to(self.device, torch.float32).contiguous(), (SHAPE_DISC_PARAMS,), 'shape disc params')
        check(self.lib.jrr_engine_set_shape_disc(self.handle, ptr(flat), self._s()), 'set_shape_disc')

    # -- operators --------------------------------------------------------------------------
    @overwrites_forward_state
    def find_joints_forward(self, betas, x6d=None, R=None, return_verts=False):
        B = self.batch
        self._chk(betas, (B, NUM_BETAS), 'betas')
        if x6d is not None:
            self._chk(x6d, (B, NUM_JOINTS, 6), 'x6d')
        if R is not None:
            self._chk(R, (B, NUM_JOINTS, 3, 3), 'R')
        joints = torch.empty(B, NUM_H36M, 3, device=self.device)
        verts = torch.empty(B, NUM_VERTS, 3, device=self.device) if return_verts else None
        check(self.lib.jrr_find_joints_forward(self.handle, ptr(x6d), ptr(R), ptr(betas), ptr(joints), ptr(verts),
                                               self._s()), 'find_joints_forward')
        return (joints, verts) if return_verts else joints

    def find_joints_backward(self, betas, djoints, x6d=None, R=None, want_dJ=False):
        B = self.batch
        self._chk(djoints, (B, NUM_H36M, 3), 'djoints')
        dx = torch.empty(B, NUM_JOINTS, 6, device=self.device) if x6d is not None else None
        dR = torch.empty(B, NUM_JOINTS, 3, 3, device=self.device) if R is not None else None
        db = torch.empty(B, NUM_BETAS, device=self.device)
        dJ = torch.empty(NUM_H36M, NUM_VERTS, device=self.device) if want_dJ else None
        check(self.lib.jrr_find_joints_backward(self.handle, ptr(x6d), ptr(R), ptr(betas), ptr(djoints), ptr(dx), ptr(dR),
                                                ptr(db), ptr(dJ), self._s()), 'find_joints_backward')
        return (dx if x6d is not None else dR), db, dJ

    @overwrites_forward_state
    def pose_disc_forward(self, x6d):
        self._chk(x6d, (self.batch, NUM_JOINTS, 6), 'x6d')
        out = torch.empty(self.batch, 25, device=self.device)
        check(self.lib.jrr_pose_disc_forward(self.handle, ptr(x6d), ptr(out), self._s()), 'pose_disc_forward')
        return out

    def pose_disc_backward_input(self, x6d, weight: float, target: float):
        dx = torch.empty(self.batch, NUM_JOINTS, 6, device=self.device)
        check(self.lib.jrr_pose_disc_backward_input(self.handle, ptr(x6d), float(weight), float(target), ptr(dx),
                                                    self._s()), 'pose_disc_backward_input')
        return dx

    @overwrites_forward_state
    def pose_disc_backward_params(self, x6d, target: float, dparams: torch.Tensor):
        """dparams += d mean((D(x)-target)^2)/d weights; returns per-pose sum_k (D-target)^2"""
        self._chk(x6d, (self.batch, NUM_JOINTS, 6), 'x6d')
        self._chk(dparams, (DISC_PARAMS,), 'dparams')
        sq = torch.empty(self.batch, device=self.device)
        check(self.lib.jrr_pose_disc_backward_params(self.handle, ptr(x6d), float(target), ptr(dparams), ptr(sq), self._s()),
              'pose_disc_backward_params')
        return sq

    def shape_disc_backward_params(self, betas, target: float, dparams: torch.Tensor):
        self._chk(betas, (self.batch, NUM_BETAS), 'betas')
        self._chk(dparams, (SHAPE_DISC_PARAMS,), 'dparams')
        sq = torch.empty(self.batch, device=self.device)
        check(self.lib.jrr_shape_disc_backward_params(self.handle, ptr(betas), float(target), ptr(dparams), ptr(sq), self._s()),
              'shape_disc_backward_params')
        return sq

    @overwrites_forward_state
    def pose_disc_vjp_params(self, x6d, gout, dparams: torch.Tensor):
        """dparams += (dD/dweights)^T gout for an upstream gradient gout (B,25); runs its own forward"""
        self._chk(x6d, (self.batch, NUM_JOINTS, 6), 'x6d')
        self._chk(gout, (self.batch, 25), 'gout')
        self._chk(dparams, (DISC_PARAMS,), 'dparams')
        check(self.lib.jrr_pose_disc_vjp_params(self.handle, ptr(x6d), ptr(gout), ptr(dparams), self._s()), 'pose_disc_vjp_params')

    def shape_disc_vjp_params(self, betas, gout, dparams: torch.Tensor):
        self._chk(betas, (self.batch, NUM_BETAS), 'betas')
        self._chk(gout, (self.batch,), 'gout')
        self._chk(dparams, (SHAPE_DISC_PARAMS,), 'dparams')
        check(self.lib.jrr_shape_disc_vjp_params(self.handle, ptr(betas), ptr(gout), ptr(dparams), self._s()), 'shape_disc_vjp_params')

    def shape_disc_forward(self, betas):
        """Shape_Discriminator.forward: betas (B,10) -> (B) sigmoid scores"""
        self._chk(betas, (self.batch, NUM_BETAS), 'betas')
        out = torch.empty(self.batch, device=self.device)
        check(self.lib.jrr_shape_disc_forward(self.handle, ptr(betas), ptr(out), self._s()), 'shape_disc_forward')
        return out

    def shape_disc_vjp_input(self, betas, gout):
        self._chk(betas, (self.batch, NUM_BETAS), 'betas')
        self._chk(gout, (self.batch,), 'gout')
        db = torch.empty(self.batch, NUM_BETAS, device=self.device)
        check(self.lib.jrr_shape_disc_vjp_input(self.handle, ptr(betas), ptr(gout), ptr(db), self._s()), 'shape_disc_vjp_input')
        return db

    def refine_aux_losses(self, pose_disc=True, shape_disc=False):
        """per-pose squared adversarial errors of the last refine_run iteration (pose: summed over the 25 outputs)"""
        pd = torch.empty(self.batch, device=self.device) if pose_disc else None
        sd = torch.empty(self.batch, device=self.device) if shape_disc else None
        check(self.lib.jrr_refine_aux_losses(self.handle, ptr(pd), ptr(sd), self._s()), 'refine_aux_losses')
        return pd, sd

    def pose_disc_vjp_input(self, x6d, gout):
        """input gradient for an arbitrary upstream gradient gout (B,25); follows pose_disc_forward"""
        self._chk(gout, (self.batch, 25), 'gout')
        dx = torch.empty(self.batch, NUM_JOINTS, 6, device=self.device)
        check(self.lib.jrr_pose_disc_vjp_input(self.handle, ptr(x6d), ptr(gout), ptr(dx), self._s()), 'pose_disc_vjp_input')
        return dx

    def find_joints_after_j_step(self, betas, x6d):
        """joints (B,17,3) of the poses of the J step that preceded (j_regressor_grad* + j_step_apply* on these very buffers) with the
        stepped regressor, from that step's stored vertices -- no second SMPL forward (jrr_find_joints_after_j_step)"""
        joints = torch.empty(self.batch, NUM_H36M, 3, device=self.device)
        check(self.lib.jrr_find_joints_after_j_step(self.handle, ptr(x6d), ptr(betas), ptr(joints), self._s()), 'find_joints_after_j_step')
        return joints

    def posed_joints(self, betas):
        """(B,24,3) posed SMPL joints (smplx J_transformed) of the most recent forward on this engine with these betas"""
        self._chk(betas, (self.batch, NUM_BETAS), 'betas')
        out = torch.empty(self.batch, NUM_JOINTS, 3, device=self.device)
        check(self.lib.jrr_smpl_posed_joints(self.handle, ptr(betas), ptr(out), self._s()), 'smpl_posed_joints')
        return out

    def posed_joints_backward(self, betas, djoints24, x6d=None, R=None):
        """adjoint of posed_joints: (B,24,3) -> (dx6d or dR, dbetas) through the kinematic chain of the most recent forward"""
        B = self.batch
        self._chk(djoints24, (B, NUM_JOINTS, 3), 'djoints24')
        dx = torch.empty(B, NUM_JOINTS, 6, device=self.device) if x6d is not None else None
        dR = torch.empty(B, NUM_JOINTS, 3, 3, device=self.device) if R is not None else None
        db = torch.empty(B, NUM_BETAS, device=self.device)
        check(self.lib.jrr_smpl_posed_joints_backward(self.handle, ptr(x6d), ptr(R), ptr(betas), ptr(djoints24), ptr(dx), ptr(dR),
                                                      ptr(db), self._s()), 'smpl_posed_joints_backward')
        return (dx if x6d is not None else dR), db

    def smpl_vertices_backward(self, betas, dverts, x6d=None, R=None):
        B = self.batch
        self._chk(dverts, (B, NUM_VERTS, 3), 'dverts')
        dx = torch.empty(B, NUM_JOINTS, 6, device=self.device) if x6d is not None else None
        dR = torch.empty(B, NUM_JOINTS, 3, 3, device=self.device) if R is not None else None
        db = torch.empty(B, NUM_BETAS, device=self.device)
        check(self.lib.jrr_smpl_vertices_backward(self.handle, ptr(x6d), ptr(R), ptr(betas), ptr(dverts), ptr(dx), ptr(dR),
                                                  ptr(db), self._s()), 'smpl_vertices_backward')
        return (dx if x6d is not None else dR), db

    def set_reprojection(self, gt_j2d=None, cam=None, cam_m=None, cam_v=None):
        """enable (tensors) / disable (None) the 2-D term of refine_run; the tensors must outlive the runs"""
        if gt_j2d is not None:
            self._chk(gt_j2d, (self.batch, NUM_H36M, 2), 'gt_j2d')
            for t, n in ((cam, 'cam'), (cam_m, 'cam_m'), (cam_v, 'cam_v')):
                self._chk(t, (self.batch, 3), n)
        self._reproj_refs = (gt_j2d, cam, cam_m, cam_v)
        check(self.lib.jrr_engine_set_reprojection(self.handle, ptr(gt_j2d), ptr(cam), ptr(cam_m), ptr(cam_v)), 'set_reprojection')

    @overwrites_forward_state
    def camera_prefit(self, x6d, betas, gt_j2d, cam, n_steps: int = 1000, lr: float = 1e-2):
        sq = torch.empty(self.batch, device=self.device)
        check(self.lib.jrr_camera_prefit(self.handle, ptr(x6d), ptr(betas), ptr(gt_j2d), ptr(cam), int(n_steps), float(lr),
                                         ptr(sq), self._s()), 'camera_prefit')
        return sq

    @overwrites_forward_state
    def silhouette_forward(self, verts, cam):
        """render_mesh alpha channel: verts (B,6890,3) in SMPL space, cam (B,3) -> (B,S,S), S = 224 (256 with FLAG_SIL_256)"""
        self._chk(verts, (self.batch, NUM_VERTS, 3), 'verts')
        self._chk(cam, (self.batch, 3), 'cam')
        alpha = torch.empty(self.batch, self.sil, self.sil, device=self.device)
        check(self.lib.jrr_silhouette_forward(self.handle, ptr(verts), ptr(cam), ptr(alpha), self._s()), 'silhouette_forward')
        return alpha

    def silhouette_backward(self, galpha):
        self._chk(galpha, (self.batch, self.sil, self.sil), 'galpha')
        dverts = torch.empty(self.batch, NUM_VERTS, 3, device=self.device)
        dcam = torch.empty(self.batch, 3, device=self.device)
        check(self.lib.jrr_silhouette_backward(self.handle, ptr(galpha), ptr(dverts), ptr(dcam), self._s()), 'silhouette_backward')
        return dverts, dcam

    def silhouette_pix_to_face(self) -> torch.Tensor:
        """(B,224,224) int32 nearest-face index per pixel (-1 = background) of the most recent rasterisation"""
        p2f = torch.empty(self.batch, self.sil, self.sil, dtype=torch.int32, device=self.device)
        check(self.lib.jrr_silhouette_pix_to_face(self.handle, ptr(p2f), self._s()), 'silhouette_pix_to_face')
        return p2f

    @overwrites_forward_state
    def silhouette_loss_grad(self, x6d, betas, cam, mask, want_dverts=True):
        """the silhouette term as the fused loop evaluates it: per-pose sum (silhouette - mask)^2, d/dverts (B,6890,3) and
        d/dcam (B,3) of 100 * mean((silhouette - mask)^2)  (jrr_silhouette_loss_grad)"""
        B = self.batch
        self._chk(x6d, (B, NUM_JOINTS, 6), 'x6d'); self._chk(betas, (B, NUM_BETAS), 'betas')
        self._chk(cam, (B, 3), 'cam'); self._chk(mask, (B, self.sil, self.sil), 'mask')
        sq = torch.empty(B, device=self.device)
        dv = torch.empty(B, NUM_VERTS, 3, device=self.device) if want_dverts else None
        dc = torch.empty(B, 3, device=self.device)
        check(self.lib.jrr_silhouette_loss_grad(self.handle, ptr(x6d), ptr(betas), ptr(cam), ptr(mask), ptr(sq), ptr(dv), ptr(dc),
                                                self._s()), 'silhouette_loss_grad')
        return sq, dv, dc

    def set_silhouette(self, mask=None, cam=None, cam_m=None, cam_v=None):
        """enable (tensors) / disable (None) the silhouette term of refine_run"""
        if mask is not None:
            self._chk(mask, (self.batch, self.sil, self.sil), 'mask')
            for t, n in ((cam, 'cam'), (cam_m, 'cam_m'), (cam_v, 'cam_v')):
                self._chk(t, (self.batch, 3), n)
        self._sil_refs = (mask, cam, cam_m, cam_v)
        check(self.lib.jrr_engine_set_silhouette(self.handle, ptr(mask), ptr(cam), ptr(cam_m), ptr(cam_v)), 'set_silhouette')

    def _refine_args(self, x6d, betas, gt_centred_mm, adam_m, adam_v, step):
        B = self.batch
        self._chk(x6d, (B, NUM_JOINTS, 6), 'x6d')
        self._chk(betas, (B, NUM_BETAS), 'betas')
        self._chk(gt_centred_mm, (B, NUM_H36M, 3), 'gt')
        self._chk(adam_m, (B, 154), 'adam_m')
        self._chk(adam_v, (B, 154), 'adam_v')
        assert step.dtype == torch.int32 and step.is_cuda

    @overwrites_forward_state
    def refine_run(self, x6d, betas, gt_centred_mm, adam_m, adam_v, step, lr: float, n_iters: int, sqerr=None,
                   after_j_step: bool = False):
        """n_iters inner iterations in ONE C call.  after_j_step=True (jrr_refine_run_after_j_step): the caller states that
        the previous call on this engine was j_regressor_grad (+ j_step_apply) on these very buffers; the first iteration
        then reuses that forward.  A mismatch the engine can detect raises instead of reusing a stale forward."""
        self._refine_args(x6d, betas, gt_centred_mm, adam_m, adam_v, step)
        fn = self.lib.jrr_refine_run_after_j_step if after_j_step else self.lib.jrr_refine_run
        check(fn(self.handle, ptr(x6d), ptr(betas), ptr(gt_centred_mm), ptr(adam_m), ptr(adam_v),
                 ptr(step), float(lr), int(n_iters), ptr(sqerr), self._s()), 'refine_run')

    @overwrites_forward_state
    def refine_run_j_steps(self, x6d, betas, gt_centred_mm, adam_m, adam_v, step, lr: float, n_iters: int, j_every: int,
                           J, J_m, J_v, J_step, j_lr: float, mask=None, sqerr=None, j_sqerr=None, after_j_step: bool = False,
                           reuse_forward: bool = True):
        """the inner loop with a J step after every j_every-th iteration, all inside ONE C call (single process only:
        there is no collective between the two halves of a J step); J / J_m / J_v / J_step are updated in place.
        reuse_forward=False: the iteration after a J step repeats its SMPL forward (include/jrr.h, after_j_step bit 1)"""
        self._refine_args(x6d, betas, gt_centred_mm, adam_m, adam_v, step)
        for t, n in ((J, 'J'), (J_m, 'J_m'), (J_v, 'J_v')):
            self._chk(t, (NUM_H36M, NUM_VERTS), n)
        assert J_step.dtype == torch.int32 and J_step.is_cuda
        check(self.lib.jrr_refine_run_j_steps(self.handle, ptr(x6d), ptr(betas), ptr(gt_centred_mm), ptr(adam_m), ptr(adam_v),
                                              ptr(step), float(lr), int(n_iters), ptr(sqerr), int(j_every), ptr(J), ptr(J_m),
                                              ptr(J_v), ptr(J_step), float(j_lr), ptr(mask), ptr(j_sqerr),
                                              int(bool(after_j_step)) | (0 if reuse_forward else 2),
                                              self._s()), 'refine_run_j_steps')

    @overwrites_forward_state
    def j_step_apply(self, J, dJ, J_m, J_v, J_step, lr: float, mask=None):
        """second half of the J step: Adam on the raw regressor with the (all-reduced) gradient + re-normalisation, one call"""
        for t, n in ((J, 'J'), (dJ, 'dJ'), (J_m, 'J_m'), (J_v, 'J_v')):
            self._chk(t, (NUM_H36M, NUM_VERTS), n)
        assert J_step.dtype == torch.int32 and J_step.is_cuda
        check(self.lib.jrr_j_step_apply(self.handle, ptr(J), ptr(dJ), ptr(J_m), ptr(J_v), ptr(J_step), float(lr), ptr(mask),
                                        self._s()), 'j_step_apply')

    def set_loss_history(self, records: int = 0, every: int = 10):
        """scripts/optimize.py:255-261: keep the five weighted loss terms of every `every`-th iteration (records = 0: off)"""
        self._hist = torch.zeros(records, 5, device=self.device) if records > 0 else None
        check(self.lib.jrr_engine_set_loss_history(self.handle, ptr(self._hist), int(records), int(every)), 'set_loss_history')

    def loss_history(self) -> Optional[torch.Tensor]:
        """(n,5) device tensor of the records written so far: [j2d/100, silhouette*100, joint*10000, poseD*10, shapeD*10]"""
        if getattr(self, '_hist', None) is None:
            return None
        return self._hist[:self.lib.jrr_engine_loss_history_count(self.handle)]

    PROF_CLASSES = ['k_prep_fwd', 'k_lbs_fwd', 'k_joints_loss', 'k_lbs_bwd', 'k_gemm_tn_blend_adjoint', 'pose_disc_gemms',
                    'k_shape_disc', 'k_prep_bwd', 'silhouette_fwd_bwd']

    def set_profiling(self, on: bool):
        check(self.lib.jrr_engine_set_profiling(self.handle, int(bool(on))), 'set_profiling')

    def profile_read(self):
        """mean ms per launch (HIP events on the launch stream) and sample counts per kernel class"""
        ms = (ctypes.c_float * 9)()
        n = (c_int32 * 9)()
        check(self.lib.jrr_engine_profile_read(self.handle, ms, n), 'profile_read')
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(self.PROF_CLASSES)}

    def probe_read(self):
        """shader-clock probe of the last profiled k_lbs_fwd launch (include/jrr.h jrr_engine_probe_read):
        (resident shader clocks of workgroup 0 / wave 0, MFMA instructions it issued, waves per SIMD, clocks per MFMA,
        the interval in ns)"""
        out = (ctypes.c_int64 * 5)()
        check(self.lib.jrr_engine_probe_read(self.handle, out), 'probe_read')
        return tuple(int(x) for x in out)

    # -- J step over the regressor's support (data parallelism: 8.7 KB instead of 468 KB per all-reduce) --------------
    J_SUPPORT_CAP = 128

    def j_support_info(self):
        """(counts per row [17], fits): positive entries of the normalised regressor per row and whether every row has at most
        128 of them.  SYNCHRONOUS; call once after set_j_regressor (J steps only shrink the support)."""
        counts = (c_int32 * NUM_H36M)()
        fits = c_int32(0)
        check(self.lib.jrr_j_support_info(self.handle, counts, byref(fits), self._s()), 'j_support_info')
        return [int(c) for c in counts], bool(fits.value)

    def support_tiles(self):
        """(active, n_tiles): whether the next joint-loss iteration runs on the regressor's support tiles only (FLAG_SUPPORT_TILES
        after j_support_info reported fits) and on how many of the 216 tiles"""
        n = c_int32(0)
        rc = self.lib.jrr_engine_support_tiles(self.handle, byref(n))
        if rc < 0:
            check(rc, 'support_tiles')
        return bool(rc), int(n.value)

    def support_vertices(self):
        """(active, n_vertices): whether those iterations run per support VERTEX, one launch per iteration and 32-pose group
        (include/jrr.h jrr_engine_support_vertices: the support has at most 64 vertices), and on how many vertices"""
        n = c_int32(0)
        rc = self.lib.jrr_engine_support_vertices(self.handle, byref(n))
        if rc < 0:
            check(rc, 'support_vertices')
        return bool(rc), int(n.value)

    @overwrites_forward_state
    def j_regressor_grad_support(self, x6d, betas, gt_centred_mm, out, sqerr=None, joints=None):
        """j_regressor_grad with the gradient delivered on the support only: out (17,128)"""
        self._chk(out, (NUM_H36M, self.J_SUPPORT_CAP), 'dJs')
        check(self.lib.jrr_j_regressor_grad_support(self.handle, ptr(x6d), ptr(betas), ptr(gt_centred_mm), ptr(out), ptr(sqerr),
                                                    ptr(joints), self._s()), 'j_regressor_grad_support')
        return out

    @overwrites_forward_state
    def j_step_apply_support(self, J, dJs, J_m, J_v, J_step, lr: float, mask=None):
        for t, n in ((J, 'J'), (J_m, 'J_m'), (J_v, 'J_v')):
            self._chk(t, (NUM_H36M, NUM_VERTS), n)
        self._chk(dJs, (NUM_H36M, self.J_SUPPORT_CAP), 'dJs')
        assert J_step.dtype == torch.int32 and J_step.is_cuda
        check(self.lib.jrr_j_step_apply_support(self.handle, ptr(J), ptr(dJs), ptr(J_m), ptr(J_v), ptr(J_step), float(lr), ptr(mask),
                                                self._s()), 'j_step_apply_support')

    @overwrites_forward_state
    def j_regressor_grad(self, x6d, betas, gt_centred_mm, sqerr=None, out=None, joints=None):
        """local dJ (first half of the J step); `out` (17,6890): write into a caller-owned buffer (e.g. a slice of the flat
        all-reduce bucket) instead of allocating; `joints` (B,17,3): receives the joints of this forward (old regressor)"""
        dJ = out if out is not None else torch.empty(NUM_H36M, NUM_VERTS, device=self.device)
        self._chk(dJ, (NUM_H36M, NUM_VERTS), 'dJ')
        if joints is not None:
            self._chk(joints, (self.batch, NUM_H36M, 3), 'joints')
        check(self.lib.jrr_j_regressor_grad(self.handle, ptr(x6d), ptr(betas), ptr(gt_centred_mm), ptr(dJ), ptr(sqerr),
                                            ptr(joints), self._s()), 'j_regressor_grad')
        return dJ


# ---- free operator functions -----------------------------------------------------------------
def rot6d_forward(x: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    x = x.contiguous().view(-1, 6)
    R = torch.empty(x.shape[0], 3, 3, device=x.device)
    check(lib.jrr_rot6d_forward(ptr(x), ptr(R), x.shape[0], stream_ptr(x.device)), 'rot6d_forward')
    return R


def rot6d_backward(x: torch.Tensor, dR: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    x = x.contiguous().view(-1, 6)
    dR = dR.contiguous()
    dx = torch.empty_like(x)
    check(lib.jrr_rot6d_backward(ptr(x), ptr(dR), ptr(dx), x.shape[0], stream_ptr(x.device)), 'rot6d_backward')
    return dx


def rodrigues_forward(aa: torch.Tensor) -> torch.Tensor:
    """smplx batch_rodrigues: axis-angle (N,3) -> (N,3,3)"""
    lib = _lib.load()
    aa = aa.contiguous().view(-1, 3).float()
    R = torch.empty(aa.shape[0], 3, 3, device=aa.device)
    check(lib.jrr_rodrigues_forward(ptr(aa), ptr(R), aa.shape[0], stream_ptr(aa.device)), 'rodrigues_forward')
    return R


def rodrigues_backward(aa: torch.Tensor, dR: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    aa = aa.contiguous().view(-1, 3).float()
    dR = dR.contiguous().float()
    daa = torch.empty_like(aa)
    check(lib.jrr_rodrigues_backward(ptr(aa), ptr(dR), ptr(daa), aa.shape[0], stream_ptr(aa.device)), 'rodrigues_backward')
    return daa


def rotmat_to_axis_angle(R: torch.Tensor) -> torch.Tensor:
    """the log map: rotation matrices (N,3,3) -> axis-angle (N,3), angle in [0, pi] (jrr_rotmat_to_axis_angle); inverts
    rodrigues_forward"""
    lib = _lib.load()
    R = R.contiguous().view(-1, 3, 3).float()
    aa = torch.empty(R.shape[0], 3, device=R.device)
    check(lib.jrr_rotmat_to_axis_angle(ptr(R), ptr(aa), R.shape[0], stream_ptr(R.device)), 'rotmat_to_axis_angle')
    return aa


def pose_export(x6d, betas, cam, index, table, status, extra=None) -> None:
    """jrr_pose_export: one launch writes the records of poses x6d (B,24,6) / betas (B,10) / cam (B,3) / extra (B,n_extra) or None
    into rows `index` (B, int64) of `table` (n_rows,240); `status` (1,) int32 collects the error bits"""
    lib = _lib.load()
    B = x6d.shape[0]
    x6d, betas, cam, index = x6d.contiguous(), betas.contiguous(), cam.contiguous(), index.contiguous()
    extra = None if extra is None else extra.contiguous()
    assert x6d.shape == (B, NUM_JOINTS, 6) and betas.shape == (B, 10) and cam.shape == (B, 3) and index.shape == (B,)
    assert table.is_contiguous() and status.is_contiguous()
    assert all(t.device == x6d.device for t in (betas, cam, index, table, status) + (() if extra is None else (extra,)))
    assert index.dtype == torch.int64 and status.dtype == torch.int32 and table.dim() == 2 and table.shape[1] == 240
    assert all(t.dtype == torch.float32 for t in (x6d, betas, cam, table))
    n_extra = 0 if extra is None else int(extra.shape[1])
    assert extra is None or (extra.shape[0] == B and extra.dtype == torch.float32)
    check(lib.jrr_pose_export(ptr(x6d), ptr(betas), ptr(cam), ptr(extra), n_extra, ptr(index), ptr(table), table.shape[0], ptr(status), B,
                              stream_ptr(x6d.device)), 'pose_export')


SMOOTH_MAX_RADIUS = 16        # include/jrr.h: JRR_SMOOTH_MAX_RADIUS


def _smooth_lists(table, order, run, status, begin, count):
    M = int(order.shape[0])
    assert table.dim() == 2 and table.shape[1] == 240 and table.dtype == torch.float32 and table.is_contiguous()
    assert order.shape == (M,) and run.shape == (M,) and order.dtype == torch.int32 and run.dtype == torch.int32
    assert order.is_contiguous() and run.is_contiguous() and status.is_contiguous() and status.dtype == torch.int32
    assert all(t.device == table.device for t in (order, run, status))
    begin = int(begin)
    count = M - begin if count is None else int(count)
    return M, begin, count


def pose_smooth(table, order, run, weights, status, begin: int = 0, count: Optional[int] = None, out=None):
    """jrr_pose_smooth: the Gaussian filter along `order` (M, int32: table rows in time order) within the runs `run` (M, int32) of a
    refined-pose `table` (n_rows,240), which is only read; `weights` (radius+1,) float32 on the device.  Computes positions
    [begin, begin + count) into `out` = (x6d (M,24,6), betas (M,10), cam (M,3), delta_deg (M,)) -- allocated, NaN-filled, when None --
    and returns it; `status` (1,) int32 collects the error bits"""
    lib = _lib.load()
    M, begin, count = _smooth_lists(table, order, run, status, begin, count)
    dev = table.device
    assert weights.dim() == 1 and weights.dtype == torch.float32 and weights.is_contiguous() and weights.device == dev
    radius = int(weights.shape[0]) - 1
    if out is None:
        out = tuple(torch.full(shape, float('nan'), device=dev) for shape in ((M, NUM_JOINTS, 6), (M, 10), (M, 3), (M,)))
    x6d, betas, cam, delta = out
    assert x6d.shape == (M, NUM_JOINTS, 6) and betas.shape == (M, 10) and cam.shape == (M, 3) and delta.shape == (M,)
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.device == dev for t in out)
    check(lib.jrr_pose_smooth(ptr(table), table.shape[0], ptr(order), ptr(run), M, ptr(weights), radius, begin, count, ptr(x6d), ptr(betas),
                              ptr(cam), ptr(delta), ptr(status), stream_ptr(dev)), 'pose_smooth')
    return out


def pose_jitter(table, order, run, status, begin: int = 0, count: Optional[int] = None, out=None) -> torch.Tensor:
    """jrr_pose_jitter: jitter_deg (M,) of positions [begin, begin + count) of `order` -- the mean over the joints of the angle of the
    rotations' second difference along the run, NaN where a position lacks a neighbour"""
    lib = _lib.load()
    M, begin, count = _smooth_lists(table, order, run, status, begin, count)
    if out is None:
        out = torch.full((M,), float('nan'), device=table.device)
    assert out.shape == (M,) and out.dtype == torch.float32 and out.is_contiguous() and out.device == table.device
    check(lib.jrr_pose_jitter(ptr(table), table.shape[0], ptr(order), ptr(run), M, begin, count, ptr(out), ptr(status),
                              stream_ptr(table.device)), 'pose_jitter')
    return out


def _view_lists(table, order, group, pair, status, begin, count):
    M = int(order.shape[0])
    assert table.dim() == 2 and table.shape[1] == 240 and table.dtype == torch.float32 and table.is_contiguous()
    assert all(t.shape == (M,) and t.dtype == torch.int32 and t.is_contiguous() and t.device == table.device for t in (order, group, pair))
    assert status.is_contiguous() and status.dtype == torch.int32 and status.device == table.device
    begin = int(begin)
    count = M - begin if count is None else int(count)
    return M, begin, count


def view_relrot_accumulate(table, order, group, pair, ref_pair, acc, status, begin: int = 0, count: Optional[int] = None):
    """jrr_view_relrot_accumulate: positions [begin, begin + count) of `order` / `group` / `pair` (M, int32: table rows sorted by scene,
    frame and camera, the (scene, frame) and the (scene, camera) of each) add the quaternion outer products of their orientation relative to
    the scene's reference camera (`ref_pair` (n_pairs,) int32) to `acc` (n_pairs, 12) int64, which the caller zeroed once; returns acc"""
    lib = _lib.load()
    M, begin, count = _view_lists(table, order, group, pair, status, begin, count)
    n_pairs = int(ref_pair.shape[0])
    assert ref_pair.shape == (n_pairs,) and ref_pair.dtype == torch.int32 and ref_pair.is_contiguous() and ref_pair.device == table.device
    assert acc.shape == (n_pairs, 12) and acc.dtype == torch.int64 and acc.is_contiguous() and acc.device == table.device
    check(lib.jrr_view_relrot_accumulate(ptr(table), table.shape[0], ptr(order), ptr(group), ptr(pair), ptr(ref_pair), n_pairs, M, begin, count,
                                         ptr(acc), ptr(status), stream_ptr(table.device)), 'view_relrot_accumulate')
    return acc


def view_fuse(table, order, group, pair, rel, cos_half_max: float, status, begin: int = 0, count: Optional[int] = None, out=None):
    """jrr_view_fuse: the views of each group fused -- `rel` (n_pairs, 4) float32 the cameras' rotations to their reference camera,
    `cos_half_max` = cos(max_deg / 2), 0 for the plain mean.  Computes positions [begin, begin + count) into `out` = (x6d (M,24,6), betas
    (M,10), delta_body_deg (M,), delta_orient_deg (M,), members (M,) int32, dropped (M,) int32) -- allocated, NaN- / zero-filled, when
    None -- and returns it; `status` (1,) int32 collects the error bits"""
    lib = _lib.load()
    M, begin, count = _view_lists(table, order, group, pair, status, begin, count)
    dev = table.device
    n_pairs = int(rel.shape[0])
    assert rel.shape == (n_pairs, 4) and rel.dtype == torch.float32 and rel.is_contiguous() and rel.device == dev
    if out is None:
        out = tuple(torch.full(shape, float('nan'), device=dev) for shape in ((M, NUM_JOINTS, 6), (M, 10), (M,), (M,))) + \
            tuple(torch.zeros(M, dtype=torch.int32, device=dev) for _ in range(2))
    x6d, betas, d_body, d_orient, members, dropped = out
    assert x6d.shape == (M, NUM_JOINTS, 6) and betas.shape == (M, 10) and all(t.shape == (M,) for t in out[2:])
    assert all(t.dtype == torch.float32 for t in out[:4]) and all(t.dtype == torch.int32 for t in out[4:])
    assert all(t.is_contiguous() and t.device == dev for t in out)
    check(lib.jrr_view_fuse(ptr(table), table.shape[0], ptr(order), ptr(group), ptr(pair), ptr(rel), n_pairs, M, float(cos_half_max), begin, count,
                            ptr(x6d), ptr(betas), ptr(d_body), ptr(d_orient), ptr(members), ptr(dropped), ptr(status), stream_ptr(dev)),
          'view_fuse')
    return out


def evaluate_joints(pred_j3d: torch.Tensor, target_j3d_mm: torch.Tensor):
    """the per-joint distances behind `evaluate`: err_j, err_pa_j (B,17) in metres (jrr_evaluate_joints)"""
    lib = _lib.load()
    B = pred_j3d.shape[0]
    pred_j3d, target_j3d_mm = pred_j3d.contiguous(), target_j3d_mm.contiguous()
    assert pred_j3d.shape == (B, 17, 3) and target_j3d_mm.shape == (B, 17, 3) and target_j3d_mm.device == pred_j3d.device
    assert pred_j3d.dtype == torch.float32 and target_j3d_mm.dtype == torch.float32
    err_j = torch.empty(B, 17, device=pred_j3d.device)
    err_pa_j = torch.empty(B, 17, device=pred_j3d.device)
    check(lib.jrr_evaluate_joints(ptr(pred_j3d), ptr(target_j3d_mm), ptr(err_j), ptr(err_pa_j), B, stream_ptr(pred_j3d.device)),
          'evaluate_joints')
    return err_j, err_pa_j


class JointRegressorTable:
    """jrr_regress_joints_prepare: 1 .. 4 raw regressors (n_reg,17,6890) (+ mask (17,6890)) normalised on the device into a workspace
    this object owns; `regress(verts)` is jrr_regress_joints: verts (B,6890,3) -> joints (n_reg,B,17,3).  No engine, no body model."""

    def __init__(self, J: torch.Tensor, mask: Optional[torch.Tensor] = None):
        lib = _lib.load()
        J = J.detach().float().contiguous()
        if J.dim() == 2:
            J = J[None]
        assert J.dim() == 3 and J.shape[1:] == (17, 6890) and 1 <= J.shape[0] <= 4, tuple(J.shape)
        self.n_reg, self.device = int(J.shape[0]), J.device
        if mask is not None:
            mask = mask.detach().float().contiguous()
            assert mask.shape == (17, 6890) and mask.device == J.device
        nbytes = int(lib.jrr_regress_joints_workspace_bytes(self.n_reg))
        self.workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=J.device)
        check(lib.jrr_regress_joints_prepare(ptr(J), self.n_reg, ptr(mask), ptr(self.workspace), self.workspace.numel() * 8,
                                             stream_ptr(J.device)), 'regress_joints_prepare')

    def regress(self, verts: torch.Tensor) -> torch.Tensor:
        lib = _lib.load()
        verts = verts.contiguous()
        B = verts.shape[0]
        assert verts.shape == (B, 6890, 3) and verts.dtype == torch.float32 and verts.device == self.device
        joints = torch.empty(self.n_reg, B, 17, 3, device=self.device)
        check(lib.jrr_regress_joints(ptr(verts), B, ptr(self.workspace), self.n_reg, ptr(joints), stream_ptr(self.device)), 'regress_joints')
        return joints


JFIT_ROW_CAP, JFIT_SPW, JFIT_MAX_WG, JFIT_INFO = 128, 32, 256, 24      # include/jrr.h: JRR_JFIT_*
NORM_UNIT, NORM_INV = 0, 1                                              # include/jrr.h: JRR_JFIT_NORM_*


class RegressorFit:
    """jrr_jfit_*: Adam steps of the J_regressor on a cache of fixed meshes (include/jrr.h).  The object owns the device state
    (support lists, raw entries, Adam moments, step counter) prepared from J_init (17,6890) and mask (17,6890) or None, and a cache of
    `n_rows` samples: `gather` fills rows of it from (B,6890,3) vertices and (B,17,3) pelvis-centred ground truth in mm, `run` enqueues
    Adam steps over consecutive minibatches, `joints` is the forward half, `dense` brings J, m and v back as (17,6890) tensors.  No
    engine, no body model."""

    def __init__(self, J_init: torch.Tensor, mask: Optional[torch.Tensor], n_rows: int):
        self.lib = _lib.load()
        J_init = J_init.detach().float().contiguous()
        assert J_init.shape == (NUM_H36M, NUM_VERTS) and J_init.is_cuda, tuple(J_init.shape)
        self.device, self.J_init = J_init.device, J_init
        if mask is not None:
            mask = mask.detach().float().contiguous()
            assert mask.shape == (NUM_H36M, NUM_VERTS) and mask.device == self.device
        self.mask = mask
        nbytes = int(self.lib.jrr_jfit_state_bytes())
        self.state = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=self.device)
        info = (c_int32 * JFIT_INFO)()
        check(self.lib.jrr_jfit_prepare(ptr(J_init), ptr(mask), ptr(self.state), self.state.numel() * 8, info, stream_ptr(self.device)),
              'jfit_prepare')
        self.ns, self.entries, self.counts = int(info[0]), int(info[1]), [int(info[4 + i]) for i in range(NUM_H36M)]
        self.n_rows = int(n_rows)
        self.row_floats = (3 * self.ns + 3 * NUM_H36M) | 1
        assert int(self.lib.jrr_jfit_cache_bytes(self.n_rows, self.ns)) == self.n_rows * self.row_floats * 4
        self.cache = torch.zeros((max(self.n_rows, 1), self.row_floats), dtype=torch.float32, device=self.device)
        self._mom_scratch = None                                   # the scratch of jrr_jfit_moments, allocated by the first call
        self._norm_scratch = None                                  # the same of jrr_jfit_norm_moments

    def info(self):
        """(NS, listed entries, Adam steps taken, entries per row); SYNCHRONOUS; raises when a call passed a foreign ns"""
        info = (c_int32 * JFIT_INFO)()
        check(self.lib.jrr_jfit_info(ptr(self.state), info, stream_ptr(self.device)), 'jfit_info')
        return int(info[0]), int(info[1]), int(info[2]), [int(info[4 + i]) for i in range(NUM_H36M)]

    def gather(self, verts: torch.Tensor, gt_centred_mm: torch.Tensor, row0: int) -> None:
        B = int(verts.shape[0])
        verts, gt = verts.contiguous(), gt_centred_mm.contiguous()
        assert verts.shape == (B, NUM_VERTS, 3) and gt.shape == (B, NUM_H36M, 3) and verts.dtype == gt.dtype == torch.float32
        assert verts.device == self.device and gt.device == self.device
        check(self.lib.jrr_jfit_gather(ptr(self.state), ptr(verts), ptr(gt), B, ptr(self.cache), self.n_rows, int(row0), self.ns,
                                       stream_ptr(self.device)), 'jfit_gather')

    def joints(self, begin: int = 0, count: Optional[int] = None) -> torch.Tensor:
        count = self.n_rows - int(begin) if count is None else int(count)
        out = torch.empty(count, NUM_H36M, 3, device=self.device)
        check(self.lib.jrr_jfit_joints(ptr(self.state), ptr(self.cache), self.n_rows, int(begin), count, self.ns, ptr(out),
                                       stream_ptr(self.device)), 'jfit_joints')
        return out

    def ground_truth_mm(self, begin: int = 0, count: Optional[int] = None) -> torch.Tensor:
        """the pelvis-centred ground truth (count,17,3) mm of cache rows [begin, begin + count)"""
        count = self.n_rows - int(begin) if count is None else int(count)
        return self.cache[begin:begin + count, 3 * self.ns:3 * self.ns + 3 * NUM_H36M].reshape(count, NUM_H36M, 3).contiguous()

    def run(self, batch: int, first: int, n_steps: int, lr: float, loss: Optional[torch.Tensor] = None, grad: Optional[torch.Tensor] = None,
            n_rows: Optional[int] = None) -> torch.Tensor:
        """n_steps Adam steps over minibatches first .. first + n_steps - 1 of the first `n_rows` cache rows (default: all); returns the
        device tensor of the steps' losses.  Nothing is read back."""
        n_rows = self.n_rows if n_rows is None else int(n_rows)
        assert 0 <= n_rows <= self.n_rows
        if loss is None:
            loss = torch.empty(max(int(n_steps), 1), device=self.device)
        assert loss.dtype == torch.float32 and loss.is_contiguous() and loss.numel() >= n_steps and loss.device == self.device
        if grad is not None:
            assert grad.shape == (NUM_H36M, JFIT_ROW_CAP) and grad.dtype == torch.float32 and grad.is_contiguous() and grad.device == self.device
        check(self.lib.jrr_jfit_run(ptr(self.state), ptr(self.cache), n_rows, self.ns, int(batch), int(first), int(n_steps), float(lr),
                                    ptr(loss), ptr(grad), stream_ptr(self.device)), 'jfit_run')
        return loss

    def dense(self):
        """(J, m, v): (17,6890) each -- the listed entries' current values over J_init and zeros"""
        J, m, v = self.J_init.clone(), torch.zeros_like(self.J_init), torch.zeros_like(self.J_init)
        check(self.lib.jrr_jfit_scatter(ptr(self.state), ptr(J), ptr(m), ptr(v), stream_ptr(self.device)), 'jfit_scatter')
        return J, m, v

    def moments(self, begin: int = 0, count: Optional[int] = None) -> torch.Tensor:
        """jrr_jfit_moments: the (W, W) float64 second moments, W = ns + 17, of cache rows [begin, begin + count) -- the sum over rows
        and axes of point w times point w' (support vertices in m, then the ground truth in mm).  Nothing is read back."""
        count = self.n_rows - int(begin) if count is None else int(count)
        W = self.ns + NUM_H36M
        if self._mom_scratch is None:
            need = ctypes.c_size_t(0)
            assert int(self.lib.jrr_jfit_moments_bytes(self.ns, ctypes.byref(need))) == W * W * 8
            self._mom_scratch = torch.empty((int(need.value) + 7) // 8, dtype=torch.float64, device=self.device)
        M = torch.empty(W, W, dtype=torch.float64, device=self.device)
        check(self.lib.jrr_jfit_moments(ptr(self.state), ptr(self.cache), self.n_rows, int(begin), count, self.ns, ptr(M),
                                        ptr(self._mom_scratch), self._mom_scratch.numel() * 8, stream_ptr(self.device)), 'jfit_moments')
        return M

    def norm_moments(self, x, mode: int, delta_m: float, begin: int = 0, count: Optional[int] = None) -> torch.Tensor:
        """jrr_jfit_norm_moments: the blocks (A_i, b_i, sum rho, sum |r|, sum w, samples; i = 1 .. 16) of cache rows
        [begin, begin + count) at the weights x as one float64 device tensor (regressor_solve.parse_norm_blocks reads it).  x: 17 rows of
        float64 weights, row i as long as the state's list of row i, or a (17,128) float64 tensor.  mode: NORM_UNIT or NORM_INV."""
        count = self.n_rows - int(begin) if count is None else int(count)
        if torch.is_tensor(x):
            xd = x.to(device=self.device, dtype=torch.float64).contiguous()
        else:
            xh = np.zeros((NUM_H36M, JFIT_ROW_CAP), dtype=np.float64)
            assert len(x) == NUM_H36M and [len(r) for r in x] == self.counts, 'x: one row of weights per list, of the list\'s length'
            for i, r in enumerate(x):
                xh[i, :len(r)] = np.asarray(r, dtype=np.float64)
            xd = torch.from_numpy(xh).to(self.device)
        assert xd.shape == (NUM_H36M, JFIT_ROW_CAP)
        if self._norm_scratch is None:
            counts = (c_int32 * NUM_H36M)(*self.counts)
            need = ctypes.c_size_t(0)
            self._norm_doubles = int(self.lib.jrr_jfit_norm_bytes(counts, ctypes.byref(need))) // 8
            assert self._norm_doubles >= 4 * (NUM_H36M - 1)
            self._norm_scratch = torch.empty((int(need.value) + 7) // 8, dtype=torch.float64, device=self.device)
        out = torch.empty(self._norm_doubles, dtype=torch.float64, device=self.device)
        check(self.lib.jrr_jfit_norm_moments(ptr(self.state), ptr(self.cache), self.n_rows, int(begin), count, self.ns, ptr(xd), int(mode),
                                             float(delta_m), ptr(out), ptr(self._norm_scratch), self._norm_scratch.numel() * 8,
                                             stream_ptr(self.device)), 'jfit_norm_moments')
        return out

    def set_entries(self, J: torch.Tensor) -> None:
        """jrr_jfit_set_entries: the raw value of every listed entry from the dense J (17,6890), zeros allowed; Adam's moments and the
        step counter start again at 0.  A listed row left without a positive entry is reported by the next info()."""
        J = J.detach().float().contiguous()
        assert J.shape == (NUM_H36M, NUM_VERTS) and J.device == self.device, tuple(J.shape)
        check(self.lib.jrr_jfit_set_entries(ptr(self.state), ptr(J), stream_ptr(self.device)), 'jfit_set_entries')


PRICE_MSE, PRICE_NORM, PRICE_DOUBLES = 0, 1, 16 * 6890 + 16 * 4         # include/jrr.h: JRR_JFIT_PRICE_*
_price_scratch = {}                                                     # (device, batch) -> the scratch of jrr_jfit_price


def price_vertices(verts: torch.Tensor, gt_centred_mm: torch.Tensor, vtx, counts, x, mode: int, delta_m: float,
                   out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """jrr_jfit_price: the sums S[i][u] (16 x 6890, joint i + 1 against every vertex u) and per joint sum r.r, sum rho, sum |r|, samples of
    the meshes verts (B,6890,3) against gt_centred_mm (B,17,3) at the lists vtx (17 rows of vertex indices, or (17,128) int32 with
    `counts`; counts None: the rows' lengths) and the float64 weights x (17 rows, or (17,128)): the (PRICE_DOUBLES,) float64 device tensor
    regressor_solve.price_gradients reads.  accumulate: ADD this batch's sums to `out`.  The lists are checked by the library on the
    host; a refusal raises before anything is launched.  No engine, no body model."""
    lib = _lib.load()
    B = int(verts.shape[0])
    verts, gt = verts.contiguous(), gt_centred_mm.contiguous()
    assert verts.shape == (B, NUM_VERTS, 3) and gt.shape == (B, NUM_H36M, 3) and verts.dtype == gt.dtype == torch.float32
    assert verts.is_cuda and gt.device == verts.device
    if counts is None:
        counts = [len(r) for r in vtx]
    ch = np.ascontiguousarray(np.asarray(counts, dtype=np.int32).reshape(NUM_H36M))
    vh, xh = np.zeros((NUM_H36M, JFIT_ROW_CAP), dtype=np.int32), np.zeros((NUM_H36M, JFIT_ROW_CAP), dtype=np.float64)
    for i in range(NUM_H36M):
        c = min(max(int(ch[i]), 0), JFIT_ROW_CAP)
        vh[i, :c] = np.asarray(vtx[i], dtype=np.int64).reshape(-1)[:c]
        xh[i, :c] = np.asarray(x[i], dtype=np.float64).reshape(-1)[:c]
    if accumulate:
        assert out is not None, 'accumulate adds to `out`'
    if out is None:
        out = torch.empty(PRICE_DOUBLES, dtype=torch.float64, device=verts.device)
    assert out.shape == (PRICE_DOUBLES,) and out.dtype == torch.float64 and out.is_contiguous() and out.device == verts.device
    key = (verts.device, B)
    if key not in _price_scratch:
        need = ctypes.c_size_t(0)
        assert int(lib.jrr_jfit_price_bytes(B, ctypes.byref(need))) == PRICE_DOUBLES * 8
        _price_scratch[key] = torch.empty((int(need.value) + 7) // 8, dtype=torch.float64, device=verts.device)
    scratch = _price_scratch[key]
    as_p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    check(lib.jrr_jfit_price(ptr(verts), ptr(gt), B, as_p(vh, c_int32), as_p(ch, c_int32), as_p(xh, ctypes.c_double), int(mode), float(delta_m),
                             1 if accumulate else 0, ptr(out), ptr(scratch), scratch.numel() * 8, stream_ptr(verts.device)), 'jfit_price')
    return out


EVAL_ACC_ROW, EVAL_ACC_TRAILER = 338, 2         # include/jrr.h: JRR_EVAL_ACC_ROW, JRR_EVAL_ACC_TRAILER


def _check_acc(acc: torch.Tensor, n_groups: int, row: int, trailer: int, dev) -> None:
    """a grouped int64 accumulator (csrc/acctab.h): contiguous, on `dev`, n_groups * row + trailer words"""
    assert acc.dtype == torch.int64 and acc.is_contiguous() and acc.device == dev
    assert acc.numel() == int(n_groups) * row + trailer


def _check_ids(ids: torch.Tensor, n: int, dev) -> None:
    """the group (or unit) ids of n poses: (n,) int32, contiguous, on `dev`"""
    assert ids.shape == (n,) and ids.dtype == torch.int32 and ids.is_contiguous() and ids.device == dev


def eval_accumulate(err_j: torch.Tensor, err_pa_j: torch.Tensor, group: torch.Tensor, n_groups: int, acc: torch.Tensor) -> None:
    """jrr_eval_accumulate: ADD the poses' per-joint errors (B,17) to rows `group` (B, int32) of the int64 table `acc`
    (n_groups * 338 + 2 words, include/jrr.h JRR_EVAL_ACC_*)"""
    lib = _lib.load()
    B = err_j.shape[0]
    err_j, err_pa_j, group = err_j.contiguous(), err_pa_j.contiguous(), group.contiguous()
    assert err_j.shape == (B, 17) and err_pa_j.shape == (B, 17) and err_j.dtype == torch.float32 and err_pa_j.dtype == torch.float32
    assert err_pa_j.device == err_j.device
    _check_ids(group, B, err_j.device)
    _check_acc(acc, n_groups, EVAL_ACC_ROW, EVAL_ACC_TRAILER, err_j.device)
    check(lib.jrr_eval_accumulate(ptr(err_j), ptr(err_pa_j), ptr(group), B, int(n_groups), ptr(acc), stream_ptr(err_j.device)),
          'eval_accumulate')


EVAL_ROOT_JOINT0, EVAL_ROOT_HIPS = 0, 1         # include/jrr.h: JRR_EVAL_ROOT_*
EVAL_TARGET_MM, EVAL_TARGET_M = 0, 1            # JRR_EVAL_TARGET_*
EVAL_MASK_ALL, EVAL_MASK_LSP14 = 0x1FFFF, 0x1FD7E      # JRR_EVAL_MASK_*


def evaluate_protocol(pred_j3d: torch.Tensor, target_j3d: torch.Tensor, joint_mask: int, root: int, target_unit: int = EVAL_TARGET_MM,
                      group: Optional[torch.Tensor] = None, n_groups: int = 1, acc: Optional[torch.Tensor] = None, rows: bool = True):
    """jrr_evaluate_protocol: the per-joint distances of the joints of `joint_mask` after centring on `root`, err_j, err_pa_j (B,17) in
    metres with +0.0 in the excluded columns (rows=False: None, None), and -- acc given -- their addition to the int64 table `acc`
    (n_groups * 338 + 2 words, include/jrr.h JRR_EVAL_ACC_*) by `group` (B, int32; None: group 0), in ONE launch.  pred (B,17,3) m,
    target (B,17,3) in `target_unit`."""
    lib = _lib.load()
    B = pred_j3d.shape[0]
    dev = pred_j3d.device
    pred_j3d, target_j3d = pred_j3d.contiguous(), target_j3d.contiguous()
    assert pred_j3d.shape == (B, 17, 3) and target_j3d.shape == (B, 17, 3) and target_j3d.device == dev
    assert pred_j3d.dtype == torch.float32 and target_j3d.dtype == torch.float32
    if group is not None:
        group = group.contiguous()
        _check_ids(group, B, dev)
    if acc is not None:
        _check_acc(acc, n_groups, EVAL_ACC_ROW, EVAL_ACC_TRAILER, dev)
    err_j, err_pa_j = (torch.empty(B, 17, device=dev), torch.empty(B, 17, device=dev)) if rows else (None, None)
    if B == 0:                                      # an empty tensor has no address to pass
        return err_j, err_pa_j
    check(lib.jrr_evaluate_protocol(ptr(pred_j3d), ptr(target_j3d), int(target_unit), int(joint_mask), int(root), ptr(group), B, int(n_groups),
                                    ptr(err_j), ptr(err_pa_j), ptr(acc), stream_ptr(dev)), 'evaluate_protocol')
    return err_j, err_pa_j


ACCEL_ACC_ROW, ACCEL_ACC_TRAILER, ACCEL_TILE = 205, 2, 32     # include/jrr.h: JRR_ACCEL_ACC_ROW, JRR_ACCEL_ACC_TRAILER, JRR_ACCEL_TILE


def accel_error(pred: torch.Tensor, gt_mm: torch.Tensor, order: torch.Tensor, run: torch.Tensor, status: torch.Tensor,
                group: Optional[torch.Tensor] = None, n_groups: int = 1, acc: Optional[torch.Tensor] = None, begin: int = 0,
                count: Optional[int] = None, out=None, rows: bool = True):
    """jrr_accel_error: the acceleration error of positions [begin, begin + count) of `order` / `run` (M, int32: rows of the tables
    `pred` (n_rows,17,3) m and `gt_mm` (n_rows,17,3) mm in time order, and each position's run).  rows: the per-position outputs
    `out` = (err_j, acc_pred_j, acc_gt_j), (M,17) each -- allocated, NaN-filled, when None -- are written and returned (rows=False:
    none, None is returned).  acc: the int64 table (n_groups * 205 + 2 words, include/jrr.h JRR_ACCEL_ACC_*) the positions are ADDED to
    by `group` (M, int32; None: group 0).  `status` (1,) int32 collects the error bit."""
    lib = _lib.load()
    M = int(order.shape[0])
    dev = pred.device
    n_rows = int(pred.shape[0])
    assert pred.shape == (n_rows, 17, 3) and gt_mm.shape == (n_rows, 17, 3) and pred.dtype == torch.float32 and gt_mm.dtype == torch.float32
    assert pred.is_contiguous() and gt_mm.is_contiguous()
    assert order.shape == (M,) and run.shape == (M,) and order.dtype == torch.int32 and run.dtype == torch.int32
    assert order.is_contiguous() and run.is_contiguous() and status.is_contiguous() and status.dtype == torch.int32
    assert all(t.device == dev for t in (gt_mm, order, run, status))
    if group is not None:
        _check_ids(group, M, dev)
    if acc is not None:
        _check_acc(acc, n_groups, ACCEL_ACC_ROW, ACCEL_ACC_TRAILER, dev)
    begin = int(begin)
    count = M - begin if count is None else int(count)
    if rows:
        if out is None:
            out = tuple(torch.full((M, 17), float('nan'), device=dev) for _ in range(3))
        assert len(out) == 3 and all(t.shape == (M, 17) and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev for t in out)
    else:
        out = None
    e, s, g = out if out is not None else (None, None, None)
    check(lib.jrr_accel_error(ptr(pred), ptr(gt_mm), n_rows, ptr(order), ptr(run), ptr(group), M, begin, count, int(n_groups), ptr(e), ptr(s),
                              ptr(g), ptr(acc), ptr(status), stream_ptr(dev)), 'accel_error')
    return out


PVE_ACC_ROW, PVE_ACC_TRAILER, PVE_MAX_PARTS, PVE_MAX_VERTS = 370, 2, 32, 65536      # include/jrr.h: JRR_PVE_ACC_ROW, JRR_PVE_ACC_TRAILER, ...


def vertex_error(pred: torch.Tensor, gt: torch.Tensor, root_pred: Optional[torch.Tensor] = None, root_gt: Optional[torch.Tensor] = None,
                 group: Optional[torch.Tensor] = None, part: Optional[torch.Tensor] = None, n_parts: int = 0, n_groups: int = 1,
                 acc: Optional[torch.Tensor] = None, acc_v: Optional[torch.Tensor] = None, means: bool = True, rows: bool = True):
    """jrr_vertex_error: the per-vertex error of meshes `pred` against `gt`, (B,n_verts,3) fp32 METRES both, after subtracting
    root_pred / root_gt (B,3; None: zero).  Returns (pve, pa_pve, err_v, err_pa_v): (B,) per-pose means in metres (means=False: None,
    None) and the (B,n_verts) distances (rows=False: None, None).  acc: the int64 group table (n_groups * 370 + 2 words, include/jrr.h
    JRR_PVE_ACC_*) the poses are ADDED to by `group` (B, int32; None: group 0), with per-part sums when `part` (n_verts, int32 labels
    in [0, n_parts)) is given; acc_v: the int64 (2,n_verts) per-vertex table the counted poses are ADDED to."""
    lib = _lib.load()
    dev = pred.device
    B, n = int(pred.shape[0]), int(pred.shape[1])
    assert pred.shape == (B, n, 3) and gt.shape == (B, n, 3) and pred.dtype == torch.float32 and gt.dtype == torch.float32
    assert pred.is_contiguous() and gt.is_contiguous() and gt.device == dev
    for r in (root_pred, root_gt):
        assert r is None or (r.shape == (B, 3) and r.dtype == torch.float32 and r.is_contiguous() and r.device == dev)
    if group is not None:
        _check_ids(group, B, dev)
    if part is not None:
        assert part.shape == (n,) and part.dtype == torch.int32 and part.is_contiguous() and part.device == dev
    if acc is not None:
        _check_acc(acc, n_groups, PVE_ACC_ROW, PVE_ACC_TRAILER, dev)
    if acc_v is not None:
        assert acc_v.dtype == torch.int64 and acc_v.is_contiguous() and acc_v.device == dev and acc_v.shape == (2, n)
    pve, pa = (torch.empty(B, device=dev), torch.empty(B, device=dev)) if means else (None, None)
    ev, epa = (torch.empty(B, n, device=dev), torch.empty(B, n, device=dev)) if rows else (None, None)
    if B == 0:                                      # an empty tensor has no address to pass
        return pve, pa, ev, epa
    check(lib.jrr_vertex_error(ptr(pred), ptr(gt), ptr(root_pred), ptr(root_gt), ptr(group), ptr(part), int(n_parts), B, n, int(n_groups),
                               ptr(pve), ptr(pa), ptr(ev), ptr(epa), ptr(acc), ptr(acc_v), stream_ptr(dev)), 'vertex_error')
    return pve, pa, ev, epa


BOOT_UNIT_ROW, BOOT_WINS_ROW, BOOT_WINS_TRAILER, BOOT_MAX_SEGMENTS = 5, 8, 3, 1025      # include/jrr.h: JRR_BOOT_*
BOOT_SUM_LIMIT = 1 << 62                        # the overflow rule of include/jrr.h: (largest count) x (largest unit word) stays below


def paired_units(before: torch.Tensor, before_pa: torch.Tensor, after: torch.Tensor, after_pa: torch.Tensor, group: torch.Tensor,
                 unit: torch.Tensor, n_groups: int, units: torch.Tensor, wins: torch.Tensor) -> None:
    """jrr_paired_units: ADD the poses' four fixed-point error sums and a 1 to rows `unit` (B, int32) of the int64 table `units`
    (n_units,5), and their better / worse / tie counts to rows `group` (B, int32) of `wins` (n_groups * 8 + 3 words, include/jrr.h
    JRR_BOOT_*).  The four inputs are the (B,17) arrays of evaluate_joints for the two regressors on the same poses."""
    lib = _lib.load()
    B = before.shape[0]
    errs = [t.contiguous() for t in (before, before_pa, after, after_pa)]
    group, unit = group.contiguous(), unit.contiguous()
    dev = errs[0].device
    assert all(t.shape == (B, 17) and t.dtype == torch.float32 and t.device == dev for t in errs)
    _check_ids(group, B, dev)
    _check_ids(unit, B, dev)
    assert units.dtype == torch.int64 and units.is_contiguous() and units.dim() == 2 and units.shape[1] == BOOT_UNIT_ROW and units.device == dev
    _check_acc(wins, n_groups, BOOT_WINS_ROW, BOOT_WINS_TRAILER, dev)
    if B == 0:                                      # an empty tensor has no address to pass
        return
    check(lib.jrr_paired_units(ptr(errs[0]), ptr(errs[1]), ptr(errs[2]), ptr(errs[3]), ptr(group), ptr(unit), B, int(n_groups), int(units.shape[0]),
                               ptr(units), ptr(wins), stream_ptr(dev)), 'paired_units')


def bootstrap_sums(units: torch.Tensor, segments, seed: int, rep_begin: int, rep_count: int, max_word: Optional[int] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """jrr_bootstrap_sums: (n_seg, rep_count, 5) int64, replicates rep_begin .. rep_begin + rep_count - 1 of every segment of the int64
    unit table `units` (n_units,5).  segments: (n_seg,2) host integers (begin, count).  max_word: the largest word of `units` where the
    caller knows it (it has the table on the host anyway); without it the table is read back once for the overflow rule, which is
    checked here in Python integers BEFORE the launch.  out: the tensor to fill (every word is stored, none is read); allocated when None."""
    lib = _lib.load()
    assert units.dtype == torch.int64 and units.is_contiguous() and units.dim() == 2 and units.shape[1] == BOOT_UNIT_ROW
    seg = np.ascontiguousarray(np.asarray(segments, dtype=np.int64).reshape(-1, 2))
    if seg.size and (np.abs(seg).max() >= 1 << 31):
        raise ValueError('bootstrap_sums: a segment word outside int32')
    seg32 = np.ascontiguousarray(seg.astype(np.int32))
    n_seg, n_units = int(seg32.shape[0]), int(units.shape[0])
    if max_word is None:
        max_word = int(units.abs().max().item()) if units.numel() else 0
    worst = (int(seg[:, 1].max()) if n_seg else 0) * int(max_word)
    if worst >= BOOT_SUM_LIMIT:
        raise OverflowError(f'bootstrap_sums: {int(seg[:, 1].max())} draws of unit words up to {int(max_word)} could reach {worst} >= 2^62')
    if out is None:
        out = torch.empty((n_seg, int(rep_count), BOOT_UNIT_ROW), dtype=torch.int64, device=units.device)
    assert out.shape == (n_seg, int(rep_count), BOOT_UNIT_ROW) and out.dtype == torch.int64 and out.is_contiguous() and out.device == units.device
    if n_seg == 0 or int(rep_count) == 0:           # an empty tensor has no address to pass
        return out
    seg_dev = torch.empty((n_seg, 2), dtype=torch.int32, device=units.device)
    check(lib.jrr_bootstrap_sums(ptr(units), n_units, c_void_p(seg32.ctypes.data), ptr(seg_dev), n_seg, int(seed) & 0xffffffffffffffff,
                                 int(rep_begin), int(rep_count), ptr(out), stream_ptr(units.device)), 'bootstrap_sums')
    return out


SHIFT_ACC_ROW, SHIFT_ACC_TRAILER = 1277, 2      # include/jrr.h: JRR_SHIFT_ACC_ROW, JRR_SHIFT_ACC_TRAILER
DISCS_MAX_SETS, DISCS_MAX_POINTS = 8, 256       # include/jrr.h: JRR_DISCS_MAX_SETS, JRR_DISCS_MAX_POINTS


def regressor_shift_accumulate(joints_a: torch.Tensor, joints_b: torch.Tensor, group: Optional[torch.Tensor], n_groups: int,
                               acc: torch.Tensor) -> None:
    """jrr_regressor_shift_accumulate: ADD the body-frame displacements joints_b - joints_a (B,17,3) m to rows `group` (B, int32; None:
    group 0) of the int64 table `acc` (n_groups * 1277 + 2 words, include/jrr.h JRR_SHIFT_ACC_*)"""
    lib = _lib.load()
    B = joints_a.shape[0]
    joints_a, joints_b = joints_a.contiguous(), joints_b.contiguous()
    assert joints_a.shape == (B, 17, 3) and joints_b.shape == (B, 17, 3)
    assert joints_a.dtype == torch.float32 and joints_b.dtype == torch.float32
    assert joints_a.is_cuda and joints_b.device == joints_a.device
    _check_acc(acc, n_groups, SHIFT_ACC_ROW, SHIFT_ACC_TRAILER, joints_a.device)
    if group is not None:
        group = group.contiguous()
        _check_ids(group, B, joints_a.device)
    check(lib.jrr_regressor_shift_accumulate(ptr(joints_a), ptr(joints_b), ptr(group), B, int(n_groups), ptr(acc),
                                             stream_ptr(joints_a.device)), 'regressor_shift_accumulate')


def draw_discs(rgb: torch.Tensor, points: torch.Tensor, colours, radius: float = 2.0, radii: Optional[torch.Tensor] = None) -> torch.Tensor:
    """jrr_draw_discs: filled discs INTO the contiguous uint8 picture `rgb` (B,h,w,3), which is returned.  points (n_sets,B,n_pts,2)
    float32 (x, y) in pixels; colours: n_sets (r, g, b) byte triples; radii (n_sets,B,n_pts) or the scalar radius.  A later set paints
    over an earlier one, a later point over an earlier one; a non-finite point or radius, or a negative radius, draws nothing."""
    lib = _lib.load()
    if not (torch.is_tensor(rgb) and rgb.dim() == 4 and rgb.shape[3] == 3 and rgb.dtype == torch.uint8 and rgb.is_cuda and rgb.is_contiguous()):
        raise ValueError('draw_discs: rgb must be a contiguous uint8 device tensor (B,h,w,3)')
    B, h, w, _ = rgb.shape
    dev = rgb.device
    if points.dim() != 4 or points.shape[1] != B or points.shape[3] != 2 or points.dtype != torch.float32 or points.device != dev:
        raise ValueError(f'draw_discs: points must be float32 (n_sets,{B},n_pts,2) on {dev}, got {tuple(points.shape)} {points.dtype}')
    points = points.contiguous()
    n_sets, n_pts = int(points.shape[0]), int(points.shape[2])
    cols = np.ascontiguousarray(np.asarray(colours, dtype=np.int64).reshape(-1, 3))
    if cols.shape[0] != n_sets or cols.min(initial=0) < 0 or cols.max(initial=0) > 255:
        raise ValueError(f'draw_discs: {n_sets} colours of three bytes each')
    cols = cols.astype(np.uint8)
    if radii is not None:
        if tuple(radii.shape) != (n_sets, B, n_pts) or radii.dtype != torch.float32 or radii.device != dev:
            raise ValueError(f'draw_discs: radii must be float32 {(n_sets, B, n_pts)} on {dev}')
        radii = radii.contiguous()
    check(lib.jrr_draw_discs(ptr(rgb), B, h, w, ptr(points), ptr(radii), float(radius), cols.ctypes.data_as(c_void_p), n_sets, n_pts,
                             stream_ptr(dev)), 'draw_discs')
    return rgb


DEPTH_MAX_POINTS, DEPTH_MAX_VERTS = 64, 8192   # include/jrr.h: JRR_DEPTH_MAX_POINTS, JRR_DEPTH_MAX_VERTS
DEPTH_ACC_ROW, DEPTH_ACC_TRAILER = 4290, 2      # include/jrr.h: JRR_DEPTH_ACC_ROW, JRR_DEPTH_ACC_TRAILER
DEPTH_STATUS_INDEX = 1


def point_mesh_depth(verts: torch.Tensor, faces: torch.Tensor, points: torch.Tensor, status: torch.Tensor, want_dist: bool = True,
                     want_wind: bool = True, want_face: bool = True):
    """jrr_point_mesh_depth: for the poses verts (B,n_verts,3) float32 m, the triangles faces (n_faces,3) int32 they share and the points
    (B,n_points,3) -- the distance to the surface (B,n_points) >= 0, the winding number of the surface around each point (inside <=>
    |wind| > 0.5; the sign is the faces' orientation) and a face that attains the distance, int32.  An output that is not wanted is None.
    status: one zeroed int32 word on the device; bit 0 is set when a face names a vertex outside [0, n_verts), read it after a
    synchronise.  One launch, nothing read back."""
    lib = _lib.load()
    if not (torch.is_tensor(verts) and verts.dim() == 3 and verts.shape[2] == 3 and verts.dtype == torch.float32 and verts.is_cuda):
        raise ValueError('point_mesh_depth: verts must be a float32 device tensor (B,n_verts,3)')
    dev, B, n_verts = verts.device, int(verts.shape[0]), int(verts.shape[1])
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32 or faces.device != dev:
        raise ValueError(f'point_mesh_depth: faces must be int32 (n_faces,3) on {dev}, got {tuple(faces.shape)} {faces.dtype} on {faces.device}')
    if points.dim() != 3 or points.shape[0] != B or points.shape[2] != 3 or points.dtype != torch.float32 or points.device != dev:
        raise ValueError(f'point_mesh_depth: points must be float32 ({B},n_points,3) on {dev}, got {tuple(points.shape)} {points.dtype}')
    if status.dtype != torch.int32 or status.numel() != 1 or status.device != dev:
        raise ValueError(f'point_mesh_depth: status must be one int32 word on {dev}')
    if not (want_dist or want_wind or want_face):
        raise ValueError('point_mesh_depth: no output wanted')
    verts, faces, points = verts.contiguous(), faces.contiguous(), points.contiguous()
    n_points, n_faces = int(points.shape[1]), int(faces.shape[0])
    dist = torch.empty((B, n_points), dtype=torch.float32, device=dev) if want_dist else None
    wind = torch.empty((B, n_points), dtype=torch.float32, device=dev) if want_wind else None
    face = torch.empty((B, n_points), dtype=torch.int32, device=dev) if want_face else None
    if B == 0:                                      # an empty tensor has no address to pass
        return dist, wind, face
    check(lib.jrr_point_mesh_depth(ptr(verts), B, n_verts, ptr(faces), n_faces, ptr(points), n_points, ptr(dist), ptr(wind), ptr(face),
                                   ptr(status), stream_ptr(dev)), 'point_mesh_depth')
    return dist, wind, face


def depth_accumulate(dist: torch.Tensor, wind: torch.Tensor, group: Optional[torch.Tensor], n_groups: int, acc: torch.Tensor) -> None:
    """jrr_depth_accumulate: ADD the signed depths of dist / wind (B,n_points), as point_mesh_depth returned them, to rows `group` (B,
    int32; None: group 0) of the int64 table `acc` (n_groups * 4290 + 2 words, include/jrr.h JRR_DEPTH_ACC_*)"""
    lib = _lib.load()
    B = int(dist.shape[0])
    dist, wind = dist.contiguous(), wind.contiguous()
    assert dist.dim() == 2 and wind.shape == dist.shape and dist.dtype == torch.float32 and wind.dtype == torch.float32
    assert dist.is_cuda and wind.device == dist.device
    _check_acc(acc, n_groups, DEPTH_ACC_ROW, DEPTH_ACC_TRAILER, dist.device)
    if group is not None:
        group = group.contiguous()
        _check_ids(group, B, dist.device)
    if B == 0:
        return
    check(lib.jrr_depth_accumulate(ptr(dist), ptr(wind), ptr(group), B, int(dist.shape[1]), int(n_groups), ptr(acc), stream_ptr(dist.device)),
          'depth_accumulate')


WINDING_MAX_POINTS = 65536                      # include/jrr.h: JRR_WINDING_MAX_POINTS
PEN_ACC_ROW, PEN_ACC_TRAILER = 55, 2            # include/jrr.h: JRR_PEN_ACC_ROW, JRR_PEN_ACC_TRAILER


def mesh_winding(verts: torch.Tensor, faces: torch.Tensor, points: torch.Tensor, status: torch.Tensor) -> torch.Tensor:
    """jrr_mesh_winding: the winding number (B,n_points) of the surface -- the poses verts (B,n_verts,3) float32 m with the triangles
    faces (n_faces,3) int32 they share -- around each of the points (B,n_points,3), up to 65 536 per pose.  The sign is the faces'
    orientation.  status: one zeroed int32 word on the device; bit 0 is set when a face names a vertex outside [0, n_verts), read it
    after a synchronise.  One launch, nothing read back."""
    lib = _lib.load()
    if not (torch.is_tensor(verts) and verts.dim() == 3 and verts.shape[2] == 3 and verts.dtype == torch.float32 and verts.is_cuda):
        raise ValueError('mesh_winding: verts must be a float32 device tensor (B,n_verts,3)')
    dev, B, n_verts = verts.device, int(verts.shape[0]), int(verts.shape[1])
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32 or faces.device != dev:
        raise ValueError(f'mesh_winding: faces must be int32 (n_faces,3) on {dev}, got {tuple(faces.shape)} {faces.dtype} on {faces.device}')
    if points.dim() != 3 or points.shape[0] != B or points.shape[2] != 3 or points.dtype != torch.float32 or points.device != dev:
        raise ValueError(f'mesh_winding: points must be float32 ({B},n_points,3) on {dev}, got {tuple(points.shape)} {points.dtype}')
    if status.dtype != torch.int32 or status.numel() != 1 or status.device != dev:
        raise ValueError(f'mesh_winding: status must be one int32 word on {dev}')
    verts, faces, points = verts.contiguous(), faces.contiguous(), points.contiguous()
    wind = torch.empty((B, int(points.shape[1])), dtype=torch.float32, device=dev)
    if B == 0:                                      # an empty tensor has no address to pass
        return wind
    check(lib.jrr_mesh_winding(ptr(verts), B, n_verts, ptr(faces), int(faces.shape[0]), ptr(points), int(points.shape[1]), ptr(wind), ptr(status),
                               stream_ptr(dev)), 'mesh_winding')
    return wind


def penetration_accumulate(wind: torch.Tensor, part: Optional[torch.Tensor], group: Optional[torch.Tensor], n_groups: int, acc: torch.Tensor,
                           per_vertex: Optional[torch.Tensor] = None, n_pen: Optional[torch.Tensor] = None,
                           n_thin: Optional[torch.Tensor] = None, n_unsure: Optional[torch.Tensor] = None) -> None:
    """jrr_penetration_accumulate: classify the winding numbers wind (B,n_verts) of the pushed vertices (penetrating, thin, unsure), write
    the per-pose counts into n_pen / n_thin / n_unsure (B, int32; each optional) and ADD the poses to rows `group` (B, int32; None: group
    0) of the int64 table `acc` (n_groups * 55 + 2 words, include/jrr.h JRR_PEN_ACC_*), by part label `part` (n_verts, int32; None: all
    part 0), and the penetrating vertices to `per_vertex` (n_verts, int64; optional)."""
    lib = _lib.load()
    assert wind.dim() == 2 and wind.dtype == torch.float32 and wind.is_cuda and wind.is_contiguous()
    B, n, dev = int(wind.shape[0]), int(wind.shape[1]), wind.device
    _check_acc(acc, n_groups, PEN_ACC_ROW, PEN_ACC_TRAILER, dev)
    assert part is None or (part.shape == (n,) and part.dtype == torch.int32 and part.is_contiguous() and part.device == dev)
    if group is not None:
        _check_ids(group, B, dev)
    assert per_vertex is None or (per_vertex.shape == (n,) and per_vertex.dtype == torch.int64 and per_vertex.is_contiguous() and per_vertex.device == dev)
    for c in (n_pen, n_thin, n_unsure):
        assert c is None or (c.shape == (B,) and c.dtype == torch.int32 and c.is_contiguous() and c.device == dev)
    if B == 0:
        return
    check(lib.jrr_penetration_accumulate(ptr(wind), ptr(part), ptr(group), B, n, int(n_groups), ptr(acc), ptr(per_vertex), ptr(n_pen), ptr(n_thin),
                                         ptr(n_unsure), stream_ptr(dev)), 'penetration_accumulate')


BONE_VALS, BONE_ACC_ROW, BONE_ACC_TRAILER = 98, 192, 2     # include/jrr.h: JRR_BONE_VALS, JRR_BONE_ACC_ROW, JRR_BONE_ACC_TRAILER


def bone_error(pred: torch.Tensor, gt_mm: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """jrr_bone_error: the (B,98) bone values of pred (B,17,3) m against gt_mm (B,17,3) mm -- 16 predicted and 16 true bone lengths
    (m), 16 angles and 16 Procrustes-rotated angles (rad), the 17 per-joint errors of the direction-only and of the length-only
    skeleton (m); include/jrr.h JRR_BONE_* has the layout and the definition.  `out`: the (B,98) tensor to fill."""
    lib = _lib.load()
    B = int(pred.shape[0])
    pred, gt_mm = pred.contiguous(), gt_mm.contiguous()
    assert pred.shape == (B, 17, 3) and gt_mm.shape == (B, 17, 3) and pred.dtype == torch.float32 and gt_mm.dtype == torch.float32
    assert pred.is_cuda and gt_mm.device == pred.device
    if out is None:
        out = torch.empty(B, BONE_VALS, device=pred.device)
    assert out.shape == (B, BONE_VALS) and out.dtype == torch.float32 and out.is_contiguous() and out.device == pred.device
    if B == 0:                                      # an empty tensor has no address to pass
        return out
    check(lib.jrr_bone_error(ptr(pred), ptr(gt_mm), B, ptr(out), stream_ptr(pred.device)), 'bone_error')
    return out


def bone_accumulate(vals: torch.Tensor, group: Optional[torch.Tensor], n_groups: int, acc: torch.Tensor) -> None:
    """jrr_bone_accumulate: ADD the poses of vals (B,98), as bone_error returned them, to rows `group` (B, int32; None: group 0) of the
    int64 table `acc` (n_groups * 192 + 2 words, include/jrr.h JRR_BONE_ACC_*)"""
    lib = _lib.load()
    B = int(vals.shape[0])
    vals = vals.contiguous()
    assert vals.shape == (B, BONE_VALS) and vals.dtype == torch.float32 and vals.is_cuda
    _check_acc(acc, n_groups, BONE_ACC_ROW, BONE_ACC_TRAILER, vals.device)
    if group is not None:
        group = group.contiguous()
        _check_ids(group, B, vals.device)
    if B == 0:
        return
    check(lib.jrr_bone_accumulate(ptr(vals), ptr(group), B, int(n_groups), ptr(acc), stream_ptr(vals.device)), 'bone_accumulate')


PLACE_ACC_ROW, PLACE_ACC_TRAILER, PLACE_MAX_ITERS = 55, 2, 64     # include/jrr.h: JRR_PLACE_ACC_ROW, JRR_PLACE_ACC_TRAILER, JRR_PLACE_MAX_ITERS


def _check_f32(t: torch.Tensor, shape, dev=None) -> torch.Tensor:
    t = t.contiguous()
    assert tuple(t.shape) == tuple(shape) and t.dtype == torch.float32 and t.is_cuda and (dev is None or t.device == dev), (t.shape, t.dtype, t.device)
    return t


def place_translation(joints: torch.Tensor, j2d: torch.Tensor, K: torch.Tensor, weight: Optional[torch.Tensor] = None, n_iters: int = 10, out=None):
    """jrr_place_translation: joints (B,17,3) m, j2d (B,17,2) full-frame pixels, K (B,3,3), weight (B,17) or None (ones) ->
    (trans (B,3) float64 m, err_lin (B,17) px, err (B,17) px, status (B,) int32); include/jrr.h has the algorithm and the
    JRR_PLACE_* status bits.  `out`: the four tensors to fill (err_lin None: not wanted)."""
    lib = _lib.load()
    B = int(joints.shape[0])
    dev = joints.device
    joints, j2d, K = _check_f32(joints, (B, 17, 3)), _check_f32(j2d, (B, 17, 2), dev), _check_f32(K, (B, 3, 3), dev)
    if weight is not None:
        weight = _check_f32(weight, (B, 17), dev)
    if not 0 <= int(n_iters) <= PLACE_MAX_ITERS:
        raise ValueError(f'place_translation: n_iters {n_iters}: 0 .. {PLACE_MAX_ITERS}')
    if out is None:
        out = (torch.empty(B, 3, dtype=torch.float64, device=dev), torch.empty(B, 17, device=dev), torch.empty(B, 17, device=dev),
               torch.empty(B, dtype=torch.int32, device=dev))
    trans, err_lin, err, status = out
    assert trans.shape == (B, 3) and trans.dtype == torch.float64 and trans.is_contiguous() and trans.device == dev
    assert status.shape == (B,) and status.dtype == torch.int32 and status.is_contiguous() and status.device == dev
    for t in (err_lin, err):
        assert t is None or (t.shape == (B, 17) and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev)
    if B == 0:                                      # an empty tensor has no address to pass
        return out
    check(lib.jrr_place_translation(ptr(joints), ptr(j2d), ptr(K), ptr(weight), B, int(n_iters), ptr(trans), ptr(err_lin), ptr(err), ptr(status),
                                    stream_ptr(dev)), 'place_translation')
    return out


def project_points(points: torch.Tensor, trans: torch.Tensor, K: torch.Tensor, want_depth: bool = False, out=None):
    """jrr_project_points: points (B,N,3) m, trans (B,3) float64, K (B,3,3) -> uv (B,N,2) pixels, NaN where Z + tz <= 0 (and, with
    want_depth, depth (B,N) = Z + tz): the 17 joints and the 6890 vertices alike.  `out`: (uv, depth or None) to fill."""
    lib = _lib.load()
    B, N = int(points.shape[0]), int(points.shape[1])
    dev = points.device
    points, K = _check_f32(points, (B, N, 3)), _check_f32(K, (B, 3, 3), dev)
    trans = trans.contiguous()
    assert trans.shape == (B, 3) and trans.dtype == torch.float64 and trans.device == dev
    if out is None:
        out = (torch.empty(B, N, 2, device=dev), torch.empty(B, N, device=dev) if want_depth else None)
    uv, depth = out
    assert uv.shape == (B, N, 2) and uv.dtype == torch.float32 and uv.is_contiguous() and uv.device == dev
    assert depth is None or (depth.shape == (B, N) and depth.dtype == torch.float32 and depth.is_contiguous() and depth.device == dev)
    if B * N:
        check(lib.jrr_project_points(ptr(points), ptr(trans), ptr(K), B, N, ptr(uv), ptr(depth), stream_ptr(dev)), 'project_points')
    return out if want_depth or depth is not None else uv


def place_accumulate(trans: torch.Tensor, err_lin: Optional[torch.Tensor], err: torch.Tensor, weight: Optional[torch.Tensor], status: torch.Tensor,
                     group: Optional[torch.Tensor], n_groups: int, acc: torch.Tensor) -> None:
    """jrr_place_accumulate: ADD the poses place_translation returned to rows `group` (B, int32; None: group 0) of the int64 table `acc`
    (n_groups * 55 + 2 words, include/jrr.h JRR_PLACE_ACC_*)"""
    lib = _lib.load()
    B = int(err.shape[0])
    dev = err.device
    err = _check_f32(err, (B, 17))
    err_lin = None if err_lin is None else _check_f32(err_lin, (B, 17), dev)
    weight = None if weight is None else _check_f32(weight, (B, 17), dev)
    trans, status = trans.contiguous(), status.contiguous()
    assert trans.shape == (B, 3) and trans.dtype == torch.float64 and trans.device == dev
    _check_ids(status, B, dev)
    _check_acc(acc, n_groups, PLACE_ACC_ROW, PLACE_ACC_TRAILER, dev)
    if group is not None:
        group = group.contiguous()
        _check_ids(group, B, dev)
    if B == 0:
        return
    check(lib.jrr_place_accumulate(ptr(trans), ptr(err_lin), ptr(err), ptr(weight), ptr(status), ptr(group), B, int(n_groups), ptr(acc),
                                   stream_ptr(dev)), 'place_accumulate')


VIS_ACC_ROW, VIS_ACC_TRAILER, VIS_MAX_POINTS = 154, 2, 65536      # include/jrr.h: JRR_VIS_ACC_ROW, JRR_VIS_ACC_TRAILER, JRR_VIS_MAX_POINTS
VIS_OCCLUDED, VIS_OUTSIDE, VIS_INVALID = 1, 2, 4                  # JRR_VIS_*: the bits of a code


def point_visibility(verts_cam: torch.Tensor, faces: torch.Tensor, points_cam: Optional[torch.Tensor], K: Optional[torch.Tensor],
                     rect: Optional[torch.Tensor], margin_m: float, min_crossings: int, status: torch.Tensor, want_count: bool = True, out=None):
    """jrr_point_visibility: per query the number of faces of the pose's own mesh -- verts_cam (B,n_verts,3) float32, camera-frame
    metres, with the triangles faces (n_faces,3) int32 -- that cross the ray from the camera centre at least margin_m in front of it,
    and its code (bit 0: count >= min_crossings, bit 1: the pixel under K (B,3,3) lies outside rect (B,4) = [x0,y0,x1,y1], bit 2:
    depth <= 0 or not finite).  points_cam (B,n_points,3), or None: the vertices themselves, the faces that name a query skipped.
    K and rect: both or neither.  status: one zeroed int32 word on the device, bit 0 for a face index out of range.
    -> (count (B,n_points) int32 or None, code (B,n_points) uint8); `out`: the two to fill.  One launch, nothing read back."""
    lib = _lib.load()
    if not (torch.is_tensor(verts_cam) and verts_cam.dim() == 3 and verts_cam.shape[2] == 3 and verts_cam.dtype == torch.float32 and verts_cam.is_cuda):
        raise ValueError('point_visibility: verts_cam must be a float32 device tensor (B,n_verts,3)')
    dev, B, n_verts = verts_cam.device, int(verts_cam.shape[0]), int(verts_cam.shape[1])
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32 or faces.device != dev:
        raise ValueError(f'point_visibility: faces must be int32 (n_faces,3) on {dev}, got {tuple(faces.shape)} {faces.dtype} on {faces.device}')
    if points_cam is not None and (points_cam.dim() != 3 or points_cam.shape[0] != B or points_cam.shape[2] != 3 or points_cam.dtype != torch.float32
                                   or points_cam.device != dev):
        raise ValueError(f'point_visibility: points_cam must be float32 ({B},n_points,3) on {dev}, got {tuple(points_cam.shape)} {points_cam.dtype}')
    if (K is None) != (rect is None):
        raise ValueError('point_visibility: K and rect go together, both or neither')
    if status.dtype != torch.int32 or status.numel() != 1 or status.device != dev:
        raise ValueError(f'point_visibility: status must be one int32 word on {dev}')
    n_points = n_verts if points_cam is None else int(points_cam.shape[1])
    if n_points > VIS_MAX_POINTS:
        raise ValueError(f'point_visibility: {n_points} points per pose: at most {VIS_MAX_POINTS}')
    if not (np.isfinite(float(margin_m)) and float(margin_m) >= 0.0) or not 1 <= int(min_crossings) <= 255:
        raise ValueError(f'point_visibility: margin_m {margin_m} must be finite and >= 0, min_crossings {min_crossings} in 1 .. 255')
    verts_cam, faces = verts_cam.contiguous(), faces.contiguous()
    points_cam = None if points_cam is None else points_cam.contiguous()
    if K is not None:
        K, rect = _check_f32(K, (B, 3, 3), dev), _check_f32(rect, (B, 4), dev)
    if out is None:
        out = (torch.empty((B, n_points), dtype=torch.int32, device=dev) if want_count else None, torch.empty((B, n_points), dtype=torch.uint8, device=dev))
    count, code = out
    assert count is None or (count.shape == (B, n_points) and count.dtype == torch.int32 and count.is_contiguous() and count.device == dev)
    assert code.shape == (B, n_points) and code.dtype == torch.uint8 and code.is_contiguous() and code.device == dev
    if B * n_points == 0:                           # an empty tensor has no address to pass
        return out
    check(lib.jrr_point_visibility(ptr(verts_cam), B, n_verts, ptr(faces), int(faces.shape[0]), ptr(points_cam), n_points, ptr(K), ptr(rect),
                                   float(margin_m), int(min_crossings), ptr(count), ptr(code), ptr(status), stream_ptr(dev)), 'point_visibility')
    return out


def visibility_accumulate(vert_code: torch.Tensor, joint_code: torch.Tensor, err_j: Optional[torch.Tensor], part: Optional[torch.Tensor],
                          pose_status: Optional[torch.Tensor], group: Optional[torch.Tensor], n_groups: int, acc: torch.Tensor,
                          per_vertex: Optional[torch.Tensor] = None) -> None:
    """jrr_visibility_accumulate: ADD the poses -- vert_code (B,n_verts) and joint_code (B,17) uint8 as point_visibility wrote them,
    err_j (B,17) float32 mm or None, pose_status (B,) int32 of place_translation or None -- to rows `group` (B, int32; None: group 0) of
    the int64 table `acc` (n_groups * 154 + 2 words, include/jrr.h JRR_VIS_ACC_*), by part label `part` (n_verts, int32; None: all part
    0), and the vertices with code 0 to `per_vertex` (n_verts, int64; optional)."""
    lib = _lib.load()
    assert vert_code.dim() == 2 and vert_code.dtype == torch.uint8 and vert_code.is_cuda and vert_code.is_contiguous()
    B, n, dev = int(vert_code.shape[0]), int(vert_code.shape[1]), vert_code.device
    assert joint_code.shape == (B, 17) and joint_code.dtype == torch.uint8 and joint_code.is_contiguous() and joint_code.device == dev
    err_j = None if err_j is None else _check_f32(err_j, (B, 17), dev)
    _check_acc(acc, n_groups, VIS_ACC_ROW, VIS_ACC_TRAILER, dev)
    assert part is None or (part.shape == (n,) and part.dtype == torch.int32 and part.is_contiguous() and part.device == dev)
    if pose_status is not None:
        _check_ids(pose_status, B, dev)
    if group is not None:
        _check_ids(group, B, dev)
    assert per_vertex is None or (per_vertex.shape == (n,) and per_vertex.dtype == torch.int64 and per_vertex.is_contiguous() and per_vertex.device == dev)
    if B == 0:
        return
    check(lib.jrr_visibility_accumulate(ptr(vert_code), ptr(joint_code), ptr(err_j), ptr(part), ptr(pose_status), ptr(group), B, n, int(n_groups),
                                        ptr(acc), ptr(per_vertex), stream_ptr(dev)), 'visibility_accumulate')


def project_joints(joints: torch.Tensor, cam: torch.Tensor) -> torch.Tensor:
    """return_2d_joints core (scripts/renderer.py:35-49): (B,17,3), (B,3) -> screen xy (B,17,2)"""
    lib = _lib.load()
    B = joints.shape[0]
    out = torch.empty(B, NUM_H36M, 2, device=joints.device)
    check(lib.jrr_project_joints(ptr(joints.contiguous()), ptr(cam.contiguous()), ptr(out), B, stream_ptr(joints.device)),
          'project_joints')
    return out


def evaluate(pred_j3d: torch.Tensor, target_j3d_mm: torch.Tensor):
    """per-pose joint error and Procrustes-aligned joint error (metres), on device"""
    lib = _lib.load()
    B = pred_j3d.shape[0]
    err = torch.empty(B, device=pred_j3d.device)
    err_pa = torch.empty(B, device=pred_j3d.device)
    check(lib.jrr_evaluate(ptr(pred_j3d.contiguous()), ptr(target_j3d_mm.contiguous()), ptr(err), ptr(err_pa), B,
                           stream_ptr(pred_j3d.device)), 'evaluate')
    return err, err_pa


def joint_loss(joints, gt_centred_mm, weight: float, batch_norm: Optional[int] = None, want_grad=True):
    lib = _lib.load()
    B = joints.shape[0]
    sq = torch.empty(B, device=joints.device)
    dj = torch.empty_like(joints) if want_grad else None
    check(lib.jrr_joint_loss(ptr(joints.contiguous()), ptr(gt_centred_mm.contiguous()), float(weight), B,
                             int(batch_norm or B), ptr(sq), ptr(dj), stream_ptr(joints.device)), 'joint_loss')
    return sq, dj


def adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    lib = _lib.load()
    assert p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous()
    check(lib.jrr_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(step), float(lr), float(beta1), float(beta2),
                            float(eps), stream_ptr(p.device)), 'adam_step')
