"""Every engine-taking entry point of include/jrr.h, held to one table: does a call between a J step's forward and its reuse DROP
that stored forward or KEEP it (csrc/engine_state.h)?

Per row and engine, at 8 poses (BP = 128: one forward workgroup column, one 64-pose backward group padded):

    1. j_regressor_grad (its _support form on engines b and c)      -- stores the forward
    2. the entry point X with valid small arguments
    3. find_joints_after_j_step on the same buffers                  -- its status is the observation: JRR_OK = X kept the forward,
                                                                        JRR_ERR_STATE = X dropped it

    engine a: KEEP_VERTS                                              (the J step stores every vertex)
    engine b: KEEP_VERTS, j_support_info called                       (the _support J step stores the support's tiles only)
    engine c: KEEP_VERTS | SUPPORT_TILES, j_support_info called       (iterations on the support's vertices)

All three also carry POSE_DISC | SHAPE_DISC | SILHOUETTE | FOLDED with both discriminators uploaded, so that every X is a valid call.
Where a row keeps the forward, the joints of step 3 must equal a fresh find_joints_forward with the current regressor.

TABLE was recorded from the commit BEFORE the engine's state moved into EngineState (observe() run against that commit's library,
printed instead of asserted) and is a literal: the refactor has to reproduce it, and a new entry point needs a row before it ships
(test_every_engine_entry_point_has_a_row parses the header)."""
import importlib
import os
import re
from ctypes import c_int32

import pytest
import torch

import oracle
from conftest import PKG_NAME, ROOT, support_tiles_available

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
B = 8
OK, ERR_STATE = 0, -4
ENGINES = ('a', 'b', 'c')

# entry point -> what engines a, b, c do with the stored forward.  None: the row cannot be observed (the call ends the engine).
TABLE = {
    'jrr_engine_destroy': None,
    'jrr_engine_set_batch_norm': ('keeps', 'keeps', 'keeps'),
    'jrr_engine_set_folded': ('drops', 'drops', 'drops'),
    'jrr_engine_set_j_regressor': ('keeps', 'drops', 'drops'),
    'jrr_engine_set_pose_disc': ('drops', 'drops', 'drops'),
    'jrr_engine_set_shape_disc': ('drops', 'drops', 'drops'),
    'jrr_find_joints_forward': ('drops', 'drops', 'drops'),
    'jrr_find_joints_backward': ('drops', 'drops', 'drops'),
    'jrr_find_joints_after_j_step': ('keeps', 'keeps', 'keeps'),
    'jrr_smpl_posed_joints': ('keeps', 'keeps', 'keeps'),
    'jrr_smpl_posed_joints_backward': ('drops', 'drops', 'drops'),
    'jrr_smpl_vertices_backward': ('drops', 'drops', 'drops'),
    'jrr_pose_disc_forward': ('drops', 'drops', 'drops'),
    'jrr_pose_disc_backward_input': ('drops', 'drops', 'drops'),
    'jrr_pose_disc_vjp_input': ('drops', 'drops', 'drops'),
    'jrr_pose_disc_backward_params': ('drops', 'drops', 'drops'),
    'jrr_pose_disc_vjp_params': ('drops', 'drops', 'drops'),
    'jrr_shape_disc_vjp_params': ('drops', 'drops', 'drops'),
    'jrr_shape_disc_backward_params': ('drops', 'drops', 'drops'),
    'jrr_shape_disc_forward': ('drops', 'drops', 'drops'),
    'jrr_shape_disc_vjp_input': ('drops', 'drops', 'drops'),
    'jrr_engine_set_reprojection': ('drops', 'drops', 'drops'),
    'jrr_camera_prefit': ('drops', 'drops', 'drops'),
    'jrr_silhouette_forward': ('drops', 'drops', 'drops'),
    'jrr_silhouette_backward': ('drops', 'drops', 'drops'),
    'jrr_silhouette_pix_to_face': ('keeps', 'keeps', 'keeps'),
    'jrr_engine_set_silhouette': ('drops', 'drops', 'drops'),
    'jrr_silhouette_loss_grad': ('drops', 'drops', 'drops'),
    'jrr_refine_run': ('drops', 'drops', 'drops'),
    'jrr_refine_aux_losses': ('drops', 'drops', 'drops'),
    'jrr_j_regressor_grad': ('keeps', 'keeps', 'keeps'),
    'jrr_j_step_apply': ('keeps', 'keeps', 'keeps'),
    'jrr_j_support_info': ('keeps', 'keeps', 'keeps'),
    'jrr_engine_support_tiles': ('keeps', 'keeps', 'keeps'),
    'jrr_engine_support_vertices': ('keeps', 'keeps', 'keeps'),
    'jrr_j_regressor_grad_support': ('keeps', 'keeps', 'keeps'),
    'jrr_j_step_apply_support': ('keeps', 'keeps', 'keeps'),
    'jrr_refine_run_after_j_step': ('drops', 'drops', 'drops'),
    'jrr_refine_run_j_steps': ('keeps', 'keeps', 'keeps'),
    'jrr_engine_set_loss_history': ('keeps', 'keeps', 'keeps'),
    'jrr_engine_loss_history_count': ('keeps', 'keeps', 'keeps'),
    'jrr_engine_info': ('keeps', 'keeps', 'keeps'),
    'jrr_engine_set_profiling': ('keeps', 'keeps', 'keeps'),
    'jrr_engine_profile_read': ('keeps', 'keeps', 'keeps'),
    'jrr_engine_probe_read': ('keeps', 'keeps', 'keeps'),
}


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


class Ctx:
    """one engine with everything a row needs; the pose buffers x6 / betas are the ones every J step and reuse names"""

    def __init__(self, kind, dm, model_np, j_np, pd, sd):
        em, sm = _mod('engine'), _mod('smpl_model')
        self.kind, self.em = kind, em
        flags = em.FLAG_KEEP_VERTS | em.FLAG_POSE_DISC | em.FLAG_SHAPE_DISC | em.FLAG_SILHOUETTE | em.FLAG_FOLDED
        if kind == 'c':
            flags |= em.FLAG_SUPPORT_TILES
        self.eng = eng = em.RefineEngine(dm, B, flags=flags)
        batch = sm.synthetic_batch(model_np, j_np, B, seed=11)
        self.x6_0, self.betas_0 = T(batch['pose6d']).to(DEV), T(batch['betas']).to(DEV)
        self.x6, self.betas = self.x6_0.clone(), self.betas_0.clone()
        self.gt = oracle.move_pelvis(T(batch['gt_j3d'])).to(DEV).contiguous()
        self.cam = T(batch['cam']).to(DEV).contiguous()
        self.cam_m, self.cam_v = torch.zeros(B, 3, device=DEV), torch.zeros(B, 3, device=DEV)
        self.gt2d = torch.zeros(B, 17, 2, device=DEV)
        self.J0 = T(j_np).to(DEV).contiguous()
        self.pd, self.sd = pd, sd
        eng.set_pose_disc(self.pd)
        eng.set_shape_disc(self.sd)
        self.dpd, self.dsd = torch.zeros(em.DISC_PARAMS, device=DEV), torch.zeros(em.SHAPE_DISC_PARAMS, device=DEV)
        self.m, self.v = torch.zeros(B, 154, device=DEV), torch.zeros(B, 154, device=DEV)
        self.step = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.dJs = torch.zeros(17, 128, device=DEV)
        self.sil_mask = torch.zeros(B, eng.sil, eng.sil, device=DEV)
        self.g25, self.g1 = torch.ones(B, 25, device=DEV), torch.ones(B, device=DEV)
        self.dj17, self.dj24 = torch.ones(B, 17, 3, device=DEV), torch.ones(B, 24, 3, device=DEV)
        self.verts = None
        self.reset()
        if kind == 'c' and support_tiles_available():
            assert eng.support_tiles()[0] and eng.support_vertices()[0]

    def reset(self):
        """the regressor of the fixture, announced from outside, and (b, c) its support reported: where every row starts"""
        self.x6.copy_(self.x6_0); self.betas.copy_(self.betas_0)
        self.J = self.J0.clone()
        self.Jm, self.Jv = torch.zeros_like(self.J), torch.zeros_like(self.J)
        self.Js = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.eng.set_j_regressor(self.J)
        if self.kind != 'a':
            assert self.eng.j_support_info()[1]

    def j_step_forward(self):
        if self.kind == 'a':
            self.dJ = self.eng.j_regressor_grad(self.x6, self.betas, self.gt)
        else:
            self.eng.j_regressor_grad_support(self.x6, self.betas, self.gt, out=self.dJs)

    def reuse_status(self, joints, x6=None):
        lib, eng = self.eng.lib, self.eng
        p = _mod('_lib').ptr
        return lib.jrr_find_joints_after_j_step(eng.handle, p(self.x6 if x6 is None else x6), p(self.betas), p(joints), eng._s())


def _refine(c, **kw):
    c.eng.refine_run(c.x6, c.betas, c.gt, c.m, c.v, c.step, 1e-2, 1, **kw)


def _refine_j_steps(c):
    c.eng.refine_run_j_steps(c.x6, c.betas, c.gt, c.m, c.v, c.step, 1e-2, 2, 2, c.J, c.Jm, c.Jv, c.Js, 1e-2)


def _j_step_apply(c):
    if c.kind == 'a':
        c.eng.j_step_apply(c.J, c.dJ, c.Jm, c.Jv, c.Js, 1e-2)
    else:      # (b, c: step 1 delivered the gradient on the support; the dense gradient buffer is a zero one)
        c.eng.j_step_apply(c.J, torch.zeros_like(c.J), c.Jm, c.Jv, c.Js, 1e-2)


def _all_verts(c):
    c.verts = c.eng.find_joints_forward(c.betas, x6d=c.x6, return_verts=True)[1]


def _rasterise(c):
    _all_verts(c)
    c.eng.silhouette_forward(c.verts, c.cam)


def _info(c):
    out = (c_int32 * 9)()
    assert c.eng.lib.jrr_engine_info(c.eng.handle, out, 9) == OK


# entry point -> (X, what must precede step 1 for X to be a valid call, what puts the engine back after step 3)
ROWS = {
    'jrr_engine_set_batch_norm': (lambda c: c.eng.set_batch_norm(B), None, None),
    'jrr_engine_set_folded': (lambda c: c.eng.set_folded(True), None, lambda c: c.eng.set_folded(False)),
    'jrr_engine_set_j_regressor': (lambda c: c.eng.set_j_regressor(c.J), None, None),
    'jrr_engine_set_pose_disc': (lambda c: c.eng.set_pose_disc(c.pd), None, None),
    'jrr_engine_set_shape_disc': (lambda c: c.eng.set_shape_disc(c.sd), None, None),
    'jrr_find_joints_forward': (lambda c: c.eng.find_joints_forward(c.betas, x6d=c.x6), None, None),
    'jrr_find_joints_backward': (lambda c: c.eng.find_joints_backward(c.betas, c.dj17, x6d=c.x6), None, None),
    'jrr_find_joints_after_j_step': (lambda c: c.eng.find_joints_after_j_step(c.betas, c.x6), None, None),
    'jrr_smpl_posed_joints': (lambda c: c.eng.posed_joints(c.betas), None, None),
    'jrr_smpl_posed_joints_backward': (lambda c: c.eng.posed_joints_backward(c.betas, c.dj24, x6d=c.x6), None, None),
    'jrr_smpl_vertices_backward': (lambda c: c.eng.smpl_vertices_backward(c.betas, torch.ones(B, 6890, 3, device=DEV), x6d=c.x6), None, None),
    'jrr_pose_disc_forward': (lambda c: c.eng.pose_disc_forward(c.x6), None, None),
    'jrr_pose_disc_backward_input': (lambda c: c.eng.pose_disc_backward_input(c.x6, 1.0, 1.0), lambda c: c.eng.pose_disc_forward(c.x6), None),
    'jrr_pose_disc_vjp_input': (lambda c: c.eng.pose_disc_vjp_input(c.x6, c.g25), lambda c: c.eng.pose_disc_forward(c.x6), None),
    'jrr_pose_disc_backward_params': (lambda c: c.eng.pose_disc_backward_params(c.x6, 1.0, c.dpd), None, None),
    'jrr_pose_disc_vjp_params': (lambda c: c.eng.pose_disc_vjp_params(c.x6, c.g25, c.dpd), None, None),
    'jrr_shape_disc_vjp_params': (lambda c: c.eng.shape_disc_vjp_params(c.betas, c.g1, c.dsd), None, None),
    'jrr_shape_disc_backward_params': (lambda c: c.eng.shape_disc_backward_params(c.betas, 1.0, c.dsd), None, None),
    'jrr_shape_disc_forward': (lambda c: c.eng.shape_disc_forward(c.betas), None, None),
    'jrr_shape_disc_vjp_input': (lambda c: c.eng.shape_disc_vjp_input(c.betas, c.g1), None, None),
    'jrr_engine_set_reprojection': (lambda c: c.eng.set_reprojection(c.gt2d, c.cam, c.cam_m, c.cam_v), None, lambda c: c.eng.set_reprojection()),
    'jrr_camera_prefit': (lambda c: c.eng.camera_prefit(c.x6, c.betas, c.gt2d, c.cam.clone(), n_steps=2), None, None),
    'jrr_silhouette_forward': (lambda c: c.eng.silhouette_forward(c.verts, c.cam), _all_verts, None),
    'jrr_silhouette_backward': (lambda c: c.eng.silhouette_backward(c.sil_mask), _rasterise, None),
    'jrr_silhouette_pix_to_face': (lambda c: c.eng.silhouette_pix_to_face(), _rasterise, None),
    'jrr_engine_set_silhouette': (lambda c: c.eng.set_silhouette(c.sil_mask, c.cam.clone(), c.cam_m, c.cam_v), None, lambda c: c.eng.set_silhouette()),
    'jrr_silhouette_loss_grad': (lambda c: c.eng.silhouette_loss_grad(c.x6, c.betas, c.cam, c.sil_mask), None, None),
    'jrr_refine_run': (_refine, None, None),
    'jrr_refine_aux_losses': (lambda c: c.eng.refine_aux_losses(True, True), _refine, None),
    'jrr_j_regressor_grad': (lambda c: c.eng.j_regressor_grad(c.x6, c.betas, c.gt), None, None),
    'jrr_j_step_apply': (_j_step_apply, None, None),
    'jrr_j_support_info': (lambda c: c.eng.j_support_info(), None, None),
    'jrr_engine_support_tiles': (lambda c: c.eng.support_tiles(), None, None),
    'jrr_engine_support_vertices': (lambda c: c.eng.support_vertices(), None, None),
    # (engine a has not been told that the support fits: there the two _support calls follow a j_support_info)
    'jrr_j_regressor_grad_support': (lambda c: c.eng.j_regressor_grad_support(c.x6, c.betas, c.gt, out=c.dJs),
                                     lambda c: c.eng.j_support_info(), None),
    'jrr_j_step_apply_support': (lambda c: c.eng.j_step_apply_support(c.J, c.dJs, c.Jm, c.Jv, c.Js, 1e-2), lambda c: c.eng.j_support_info(), None),
    'jrr_refine_run_after_j_step': (lambda c: _refine(c, after_j_step=True), None, None),
    'jrr_refine_run_j_steps': (_refine_j_steps, None, None),
    'jrr_engine_set_loss_history': (lambda c: c.eng.set_loss_history(4, 1), None, lambda c: c.eng.set_loss_history(0)),
    'jrr_engine_loss_history_count': (lambda c: c.eng.lib.jrr_engine_loss_history_count(c.eng.handle), None, None),
    'jrr_engine_info': (_info, None, None),
    'jrr_engine_set_profiling': (lambda c: c.eng.set_profiling(True), None, lambda c: c.eng.set_profiling(False)),
    'jrr_engine_profile_read': (lambda c: c.eng.profile_read(), None, None),
    'jrr_engine_probe_read': (lambda c: c.eng.probe_read(), None, None),
}


def observe(c, name):
    """steps 1 - 3 for entry point `name` on engine context c: ('keeps' | 'drops', the joints of step 3)"""
    call, before, after = ROWS[name]
    c.reset()
    if before:
        before(c)
    c.j_step_forward()
    call(c)
    joints = torch.empty(B, 17, 3, device=DEV)
    rc = c.reuse_status(joints)
    assert rc in (OK, ERR_STATE), f'{name} on engine {c.kind}: find_joints_after_j_step returned {rc}'
    if after:
        after(c)
    return ('keeps' if rc == OK else 'drops'), joints


def header_entry_points():
    with open(os.path.join(ROOT, 'include', 'jrr.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    return [m.group(1) for m in re.finditer(r'\b(\w+)\s*\(\s*(?:const\s+)?jrr_engine_t\s*\*', text)]


@pytest.fixture(scope='module')
def contexts(smpl_model_np, j_h36m_np):
    em = _mod('engine')
    dm = em.DeviceModel(smpl_model_np, DEV)
    pd = em.flatten_state_dict(oracle.formula_state_dict(oracle.DISC_PARAM_SHAPES, seed=0), em.DISC_KEYS).to(DEV)
    sd = em.flatten_state_dict(oracle.formula_state_dict(oracle.SHAPE_DISC_PARAM_SHAPES, seed=1), em.SHAPE_DISC_KEYS).to(DEV)
    return {k: Ctx(k, dm, smpl_model_np, j_h36m_np, pd, sd) for k in ENGINES}


def test_every_engine_entry_point_has_a_row():
    names = header_entry_points()
    assert len(names) >= 45 and len(set(names)) == len(names)
    missing = [n for n in names if n not in TABLE]
    assert not missing, f'no row says "drops" or "keeps" for {missing}'
    assert sorted(n for n, row in TABLE.items() if row is not None) == sorted(ROWS)
    assert all(row is None or (len(row) == 3 and set(row) <= {'keeps', 'drops'}) for row in TABLE.values())


@pytest.mark.parametrize('name', sorted(ROWS))
def test_entry_point_keeps_or_drops_the_stored_forward(contexts, name):
    for i, kind in enumerate(ENGINES):
        c = contexts[kind]
        got, joints = observe(c, name)
        assert got == TABLE[name][i], f'{name} on engine {kind}: {got}, the table says {TABLE[name][i]}'
        if got == 'keeps':      # bound of test_gpu_round5.py::test_find_joints_after_j_step_equals_a_fresh_forward
            fresh = c.eng.find_joints_forward(c.betas, x6d=c.x6)
            assert (joints - fresh).abs().max().item() < 2e-6, f'{name} on engine {kind}'


def test_reuse_with_other_buffers_is_refused(contexts):
    lib_mod = _mod('_lib')
    for kind in ENGINES:
        c = contexts[kind]
        c.reset()
        c.j_step_forward()
        other = c.x6.clone()
        with pytest.raises(lib_mod.JrrError, match='same pose buffers'):
            c.eng.refine_run(other, c.betas, c.gt, c.m, c.v, c.step, 1e-2, 1, after_j_step=True)
        # (refused before anything was touched: the forward is still there for the buffers it belongs to)
        joints = torch.empty(B, 17, 3, device=DEV)
        assert c.reuse_status(joints, x6=other) == ERR_STATE
        assert c.reuse_status(joints) == OK


def test_outside_regressor_after_a_j_step(contexts):
    """jrr_engine_set_j_regressor between a J step and its reuse: refused after a partial-vertex step (the stored tiles are those of
    the OLD support), accepted after a full-vertex one (the vertices do not depend on the regressor)"""
    lib_mod = _mod('_lib')
    for kind in ENGINES:
        c = contexts[kind]
        c.reset()
        c.j_step_forward()
        _j_step_apply(c)
        c.eng.set_j_regressor(c.J)
        if kind == 'a':
            c.eng.refine_run(c.x6, c.betas, c.gt, c.m, c.v, c.step, 1e-2, 1, after_j_step=True)
        else:
            with pytest.raises(lib_mod.JrrError, match='same pose buffers'):
                c.eng.refine_run(c.x6, c.betas, c.gt, c.m, c.v, c.step, 1e-2, 1, after_j_step=True)


def test_j_step_with_another_mask_turns_the_support_tiles_off(contexts):
    c = contexts['c']
    c.reset()
    if support_tiles_available():
        assert c.eng.support_tiles()[0]
    c.j_step_forward()
    c.eng.j_step_apply(c.J, torch.zeros_like(c.J), c.Jm, c.Jv, c.Js, 1e-2, mask=torch.ones_like(c.J))
    assert c.eng.support_tiles() == (False, 216) and c.eng.support_vertices() == (False, 0)
    joints = torch.empty(B, 17, 3, device=DEV)
    assert c.reuse_status(joints) == ERR_STATE      # ... and the step's partial vertices serve no product any more
