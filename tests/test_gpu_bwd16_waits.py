"""k_lbs_bwd16 keeps its register prefetch in flight with hand-counted vmcnt waits (csrc/lbs_bwd.hip, csrc/jrr_common.h quad_load /
quads_landed).  A count that is too large is a DATA HAZARD -- a product reads a register whose load has not landed -- and shows as
wrong or non-repeatable numbers, not as a fault.  So every case here runs TWICE and must be bitwise equal to itself, and is held
against the oracle with the bounds tests/test_gpu_round4.py uses for the same quantities.  The shapes reach the edges of the
counting: a partial and a full 64-pose group, chunk counts that give 6 tiles per chunk / uneven odd and even tile counts / one
216-tile chunk that crosses every segment change (a flush in mid-loop), the tile-listed kernel with 0 .. 3 tiles per chunk, a
wide tile, 12 joint slots, and both kinds of outside vertex adjoint (which add six loads per tile to the in-order stream).
The assembly side of the same change: tests/test_waitcnt_codegen.py."""
import importlib
import os

import numpy as np
import pytest
import torch

import oracle
from conftest import PKG_NAME, support_tiles_available

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
KNOBS = ('JRR_DENSE_SKINNING', 'JRR_SKIN_JOINTS', 'JRR_VERTEX_ORDER', 'JRR_BWD16', 'JRR_NVCB16')


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _fresh_state(B):
    return (torch.zeros(B, 154, device=DEV), torch.zeros(B, 154, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))


def _relerr(a, b):
    return ((a.cpu().double() - b.double()).abs().max() / b.double().abs().max()).item()


class _env:
    """knobs read by jrr_model_create / jrr_engine_create from the environment as it is at that moment"""
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        if any(k in os.environ for k in KNOBS):
            pytest.skip('the suite itself runs under a forced kernel variant')
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k in self.kv:
            os.environ.pop(k, None)


_models = {}


def _device_model(kind, smpl_model_np, j_h36m_np):
    """(numpy model, DeviceModel) of a body, built once per session"""
    if kind not in _models:
        sm, em = _mod('smpl_model'), _mod('engine')
        model = sm.with_wide_tile(smpl_model_np, 100, 13) if kind == 'wide13' else smpl_model_np
        env = {'JRR_SKIN_JOINTS': '12'} if kind == 'skin12' else {}
        hint = np.nonzero((j_h36m_np > 0).any(0))[0] if kind == 'hinted' else None
        with _env(**env):
            dm = em.DeviceModel(model, DEV, hint_vertices=hint)
        assert dm.info['joint_slots'] == (12 if kind == 'skin12' else 8), dm.info
        assert (dm.info['wide_tiles'] > 0) == (kind == 'wide13'), dm.info
        _models[kind] = (model, dm)
    return _models[kind]


_refs = {}


def _find_joints_reference(model, J, B):
    """float64 oracle: joints, vertices and the gradients of sum(joints * dj) -- computed once per (body, batch), never changed"""
    key = (id(model), B)
    if key not in _refs:
        sm = _mod('smpl_model')
        batch = sm.synthetic_batch(model, J, B, seed=40 + B)
        x6d, betas = T(batch['pose6d']).double(), T(batch['betas']).double()
        dj = torch.randn(B, 17, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        Jt = T(J).double().requires_grad_(True)
        smpl = oracle.OracleSMPL(model, dtype=torch.float64)
        xr, br = x6d.clone().requires_grad_(True), betas.clone().requires_grad_(True)
        R = oracle.rot6d_to_rotmat(xr.reshape(-1, 6)).view(B, 24, 3, 3)
        ref_j, ref_v = oracle.find_joints(smpl, br, R[:, :1], R[:, 1:], Jt, mask=oracle.find_j_reg_mask(Jt.detach()), return_verts=True)
        (ref_j * dj).sum().backward()
        _refs[key] = dict(x6d=x6d, betas=betas, dj=dj, joints=ref_j.detach(), verts=ref_v.detach(), dx=xr.grad, db=br.grad, dJ=Jt.grad)
    return _refs[key]


# (body, JRR_NVCB16 or None = the engine's own choice): chunks of 6 tiles; 35 chunks = 6 or 7 tiles, odd and even counts; ONE chunk of
# 216 tiles, across every segment change; the engine's own geometry; the same on the wide-tile body and with the 12-slot kernels
FIND_JOINTS_CASES = [('surface', '36'), ('surface', '35'), ('surface', '1'), ('surface', None), ('wide13', None), ('wide13', '35'),
                     ('skin12', None), ('skin12', '1')]


@pytest.mark.parametrize('B', [37, 64])
@pytest.mark.parametrize('kind,nvcb16', FIND_JOINTS_CASES)
def test_find_joints_backward_vs_oracle_and_itself(smpl_model_np, j_h36m_np, kind, nvcb16, B):
    model, dm = _device_model(kind, smpl_model_np, j_h36m_np)
    em = _mod('engine')
    ref = _find_joints_reference(model, j_h36m_np, B)
    with _env(**({'JRR_NVCB16': nvcb16} if nvcb16 else {})):
        eng = em.RefineEngine(dm, B, flags=em.FLAG_KEEP_VERTS)
    eng.set_j_regressor(T(j_h36m_np))
    xd, bd = ref['x6d'].float().contiguous().to(DEV), ref['betas'].float().contiguous().to(DEV)
    djd = ref['dj'].float().to(DEV)
    runs = []
    for _ in range(2):
        joints, verts = eng.find_joints_forward(bd, x6d=xd, return_verts=True)
        dx, db, dJ = eng.find_joints_backward(bd, djd, x6d=xd, want_dJ=True)
        runs.append([t.cpu().numpy().copy() for t in (joints, verts, dx, db, dJ)])
    assert (verts.cpu().double() - ref['verts']).abs().max().item() < 2e-5
    assert (joints.cpu().double() - ref['joints']).abs().max().item() < 2e-5
    errs = (_relerr(dx, ref['dx']), _relerr(db, ref['db']), _relerr(dJ, ref['dJ']))
    print(kind, nvcb16, B, 'relative errors dx6d / dbetas / dJ:', errs)
    assert max(errs) < 2e-4, errs
    assert (dJ.cpu()[T(j_h36m_np) <= 0] == 0).all()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('B', [37, 64])
@pytest.mark.parametrize('kind', ['surface', 'skin12'])
def test_outside_vertex_adjoint_alone_vs_oracle_and_itself(smpl_model_np, j_h36m_np, kind, B):
    """smpl_vertices_backward: the caller's vertex adjoint and nothing else (six more loads per tile, no joint adjoint)"""
    model, dm = _device_model(kind, smpl_model_np, j_h36m_np)
    em = _mod('engine')
    ref = _find_joints_reference(model, j_h36m_np, B)
    dv = torch.randn(B, 6890, 3, generator=torch.Generator().manual_seed(6), dtype=torch.float64) * 1e-3
    smpl = oracle.OracleSMPL(model, dtype=torch.float64)
    xr, br = ref['x6d'].clone().requires_grad_(True), ref['betas'].clone().requires_grad_(True)
    R = oracle.rot6d_to_rotmat(xr.reshape(-1, 6)).view(B, 24, 3, 3)
    (smpl(R[:, :1], R[:, 1:], br).vertices * dv).sum().backward()
    eng = em.RefineEngine(dm, B, flags=em.FLAG_KEEP_VERTS)
    eng.set_j_regressor(T(j_h36m_np))
    xd, bd = ref['x6d'].float().contiguous().to(DEV), ref['betas'].float().contiguous().to(DEV)
    dvd = dv.float().contiguous().to(DEV)
    runs = []
    for _ in range(2):
        eng.find_joints_forward(bd, x6d=xd, return_verts=True)
        dx, db = eng.smpl_vertices_backward(bd, dvd, x6d=xd)
        runs.append((dx.cpu().numpy().copy(), db.cpu().numpy().copy()))
    errs = (_relerr(dx, xr.grad), _relerr(db, br.grad))
    print(kind, B, 'relative errors dx6d / dbetas:', errs)
    assert max(errs) < 2e-4, errs
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def _wide_support_regressor():
    """17 x 6 = 102 support vertices: more than the per-vertex iteration is built for, so FLAG_SUPPORT_TILES runs the TILE LISTS
    (k_lbs_bwd16<.., LIST>) whatever JRR_SUPPORT_FUSED says -- that knob is read once per process and cannot be set from a test"""
    rng = np.random.RandomState(11)
    J = np.zeros((17, 6890), np.float32)
    cols = rng.choice(6890, 17 * 6, replace=False).reshape(17, 6)
    for i in range(17):
        J[i, cols[i]] = rng.dirichlet(np.ones(6)).astype(np.float32)
    return J


@pytest.mark.parametrize('B', [37, 64])
@pytest.mark.parametrize('regressor', ['wide102', 'h36m'])
@pytest.mark.parametrize('hinted', [False, True])
def test_listed_tiles_three_iterations_vs_oracle_and_itself(smpl_model_np, j_h36m_np, hinted, regressor, B):
    """the tile-listed kernel: the chunks of a list of a few tiles get 0, 1, 2 or 3 of them (a hinted body: a handful of tiles, most
    chunks empty).  With the shipped regressor (56 support vertices) the lists run when the process was started with
    JRR_SUPPORT_FUSED=0 and the per-vertex iteration otherwise; the 102-vertex regressor always runs the lists."""
    sm, em = _mod('smpl_model'), _mod('engine')
    J = _wide_support_regressor() if regressor == 'wide102' else j_h36m_np
    with _env():
        dm = em.DeviceModel(smpl_model_np, DEV, hint_vertices=np.nonzero((J > 0).any(0))[0] if hinted else None)
    batch = sm.synthetic_batch(smpl_model_np, J, B, seed=17 + B)
    x6, betas = T(batch['pose6d']), T(batch['betas'])
    gt_c = oracle.move_pelvis(T(batch['gt_j3d']))
    o, p, b_, _ = oracle.refine_poses(oracle.OracleSMPL(smpl_model_np), T(J), x6[:, :1], x6[:, 1:], betas, gt_c, 3)
    eng = em.RefineEngine(dm, B, flags=em.FLAG_KEEP_VERTS | em.FLAG_SUPPORT_TILES)
    eng.set_j_regressor(T(J))
    assert eng.j_support_info()[1]
    assert eng.support_tiles()[0] == support_tiles_available()
    if regressor == 'wide102':
        assert eng.support_vertices() == (False, 0)
    runs = []
    for _ in range(2):
        xd, bd = x6.to(DEV).contiguous(), betas.to(DEV).contiguous()
        m, vv, step = _fresh_state(B)
        eng.refine_run(xd, bd, gt_c.to(DEV).contiguous(), m, vv, step, 1e-2, 3)
        runs.append((xd.cpu().numpy().copy(), bd.cpu().numpy().copy()))
    d = (xd.cpu() - torch.cat([o, p], 1)).abs()
    print(regressor, hinted, B, 'pose error max / mean:', d.max().item(), d.mean().item(), 'betas:', (bd.cpu() - b_).abs().max().item())
    assert d.max().item() < 6e-4 and d.mean().item() < 1e-5, (d.max().item(), d.mean().item())
    assert (bd.cpu() - b_).abs().max().item() < 3e-4
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_silhouette_loop_with_both_adjoints_vs_oracle_and_itself(smpl_model_np, j_h36m_np):
    """the fused silhouette loop hands k_lbs_bwd16 the joint adjoint AND an outside vertex adjoint (DV = 2): two iterations at a
    partial pose group against oracle.refine_poses(sil_mask=...), poses and betas within the bounds tests/test_gpu_round3.py holds
    the same loop to (2e-3 max, 1e-4 mean), bitwise repeatable"""
    from oracle import silhouette_port as sp
    sm, em = _mod('smpl_model'), _mod('engine')
    B, n = 9, 2
    batch = sm.synthetic_batch(smpl_model_np, j_h36m_np, B, seed=57)
    x6, betas, cam0 = T(batch['pose6d']), T(batch['betas']), T(batch['cam'])
    smpl = oracle.OracleSMPL(smpl_model_np)
    R = oracle.rot6d_to_rotmat(x6.reshape(-1, 6)).view(B, 24, 3, 3)
    verts = smpl(R[:, :1], R[:, 1:], betas).vertices
    faces = smpl_model_np['faces']
    mask = (sp.soft_silhouette(verts, faces, cam0 + torch.tensor([0.15, -0.1, 1.0]))[:, 0] > 0).float()
    gt_c = oracle.move_pelvis(T(batch['gt_j3d']))
    o, p, b, _, _ = oracle.refine_poses(smpl, T(j_h36m_np), x6[:, :1], x6[:, 1:], betas, gt_c, n, cam=cam0, sil_mask=mask[:, None], faces=faces)
    _, dm = _device_model('surface', smpl_model_np, j_h36m_np)
    eng = em.RefineEngine(dm, B, flags=em.FLAG_SILHOUETTE | em.FLAG_KEEP_VERTS)
    eng.set_j_regressor(T(j_h36m_np))
    md, gd = mask.to(DEV).contiguous(), gt_c.to(DEV).contiguous()
    runs = []
    for _ in range(2):
        xd, bd, cd = x6.clone().to(DEV), betas.clone().to(DEV), cam0.clone().to(DEV)
        cm, cv = torch.zeros(B, 3, device=DEV), torch.zeros(B, 3, device=DEV)
        eng.set_silhouette(md, cd, cm, cv)
        m, v, step = _fresh_state(B)
        eng.refine_run(xd, bd, gd, m, v, step, 1e-2, n)
        eng.set_silhouette(None)
        runs.append([t.cpu().numpy().copy() for t in (xd, bd, cd)])
    dx = (xd.cpu() - torch.cat([o, p], 1)).abs()
    db = (bd.cpu() - b).abs()
    print('silhouette loop: pose error max / mean', dx.max().item(), dx.mean().item(), 'betas', db.max().item(), db.mean().item())
    assert dx.max().item() < 2e-3 and dx.mean().item() < 1e-4, (dx.max().item(), dx.mean().item())
    assert db.max().item() < 2e-3 and db.mean().item() < 1e-4, (db.max().item(), db.mean().item())
    for a, b_ in zip(*runs):
        assert np.array_equal(a, b_)
