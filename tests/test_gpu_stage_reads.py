"""The chunk boundary of k_disc_gemm (next chunk's barrier and first operand reads inside the last quad pair), its batched epilogue loads
and the global-address stores of k_lbs_fwd / k_blend_adjoint / the per-joint MLP kernels, at the smallest shapes at which they can go
wrong (tests/test_stage_reads_codegen.py reads the generated code):

  * the discriminator's products at 128 and 192 poses -- K = 768 and 1024 are 24 and 32 chunks around the three-slot ring, i.e. two
    residues of the chunk count modulo the ring, with the boundary inside the last quad pair of every chunk but the
    last; the 64 x 32 tile (engines below 2048 pose columns) against the oracle and, bit for bit, against the 128 x 64 tile of a
    4096-pose engine;
  * k_lbs_fwd at B = 128 and B = 130 (the second pads to 256 pose columns: a pose group of padding): vertices, joints and the
    v_posed-consuming backward against the float64 oracle for the 8-slot, 12-slot, dense and wide-tile kernels, three iterations of the
    loop (blend adjoint included) for those and for the tile-listed kernels, and the engine's workspace -- the vertex buffer with its
    padded pose columns in it -- bit-identical from one call to the next.
The tolerances are those of tests/test_gpu_parity.py, tests/test_gpu_round4.py and tests/test_gpu_bwd16_waits.py."""
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
KNOBS = ('JRR_DENSE_SKINNING', 'JRR_SKIN_JOINTS', 'JRR_VERTEX_ORDER', 'JRR_BWD16')


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _relerr(a, b):
    return ((a.cpu().double() - b.double()).abs().max() / b.double().abs().max()).item()


# ---- discriminator ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def disc(smpl_model_np):
    """the 192 test poses, the oracle's outputs and input gradients for the first 128 and for all 192 (computed once), and what a
    4096-pose engine (128 x 64 tiles) makes of them as its first columns"""
    em = _mod('engine')
    dm = em.DeviceModel(smpl_model_np, DEV)
    sd = oracle.formula_state_dict(oracle.DISC_PARAM_SHAPES, seed=0)
    flat = em.flatten_state_dict(sd, em.DISC_KEYS)
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(4096, 24, 6, generator=gen) * 0.7
    ref = {}
    for B in (128, 192):
        xr = x[:B].clone().requires_grad_(True)
        out = oracle.discriminator_forward(sd, xr)
        (((out - 1) ** 2).sum() / (4096 * 25) * 10.0).backward()      # weight 10, target 1, mean over the batch norm of 4096 poses
        ref[B] = (out.detach().numpy()[:, :, 0], xr.grad.clone())
    big = em.RefineEngine(dm, 4096, flags=em.FLAG_POSE_DISC)
    big.set_pose_disc(flat)
    xd = x.to(DEV).contiguous()
    big_out = big.pose_disc_forward(xd).cpu()
    big_dx = big.pose_disc_backward_input(xd, 10.0, 1.0).cpu()
    del big
    return dict(em=em, dm=dm, flat=flat, x=x, ref=ref, big_out=big_out, big_dx=big_dx)


@pytest.mark.parametrize('B', [128, 192])
def test_disc_products_at_one_and_two_column_tiles_vs_oracle_and_the_wide_tile(disc, B):
    em = disc['em']
    eng = em.RefineEngine(disc['dm'], B, batch_norm=4096, flags=em.FLAG_POSE_DISC)
    eng.set_pose_disc(disc['flat'])
    xd = disc['x'][:B].to(DEV).contiguous()
    out = eng.pose_disc_forward(xd).cpu()
    dx = eng.pose_disc_backward_input(xd, 10.0, 1.0).cpu()
    ref_out, ref_dx = disc['ref'][B]
    np.testing.assert_allclose(out.numpy(), ref_out, rtol=0, atol=3e-6)
    assert ((dx - ref_dx).abs().max() / ref_dx.abs().max()).item() < 5e-4
    # the same columns of the 4096-pose engine: another tile shape, the same operations per output element
    assert torch.equal(out, disc['big_out'][:B])
    assert torch.equal(dx, disc['big_dx'][:B])
    # the 128 x 64 tile against the oracle as well
    np.testing.assert_allclose(disc['big_out'][:B].numpy(), ref_out, rtol=0, atol=3e-6)
    assert ((disc['big_dx'][:B] - ref_dx).abs().max() / ref_dx.abs().max()).item() < 5e-4


# ---- LBS forward -----------------------------------------------------------------------------------------------------------------
BODIES = {       # id -> (environment of jrr_model_create, wide-tile body?, joint slots)
    'slots8': ({}, False, 8),
    'slots12': ({'JRR_SKIN_JOINTS': '12'}, False, 12),
    'dense': ({'JRR_DENSE_SKINNING': '1'}, False, 0),
    'wide13': ({}, True, 8),
}
_bodies, _refs = {}, {}


def _body(kind, smpl_model_np):
    if any(k in os.environ for k in KNOBS):
        pytest.skip('the suite itself runs under a forced kernel variant')
    if kind not in _bodies:
        sm, em = _mod('smpl_model'), _mod('engine')
        env, wide, slots = BODIES[kind]
        model = sm.with_wide_tile(smpl_model_np, 100, 13) if wide else smpl_model_np
        os.environ.update(env)          # read by jrr_model_create
        try:
            dm = em.DeviceModel(model, DEV)
        finally:
            for k in env:
                os.environ.pop(k, None)
        assert dm.info['joint_slots'] == slots and (dm.info['wide_tiles'] > 0) == wide, dm.info
        _bodies[kind] = (model, dm)
    return _bodies[kind]


def _reference(model, wide, J, B):
    """float64 oracle of find_joints and its gradients, fp32 oracle of three iterations -- once per (body, batch), never changed"""
    key = (wide, B, id(J))
    if key not in _refs:
        sm = _mod('smpl_model')
        batch = sm.synthetic_batch(model, J, B, seed=90 + B)
        x6, betas = T(batch['pose6d']), T(batch['betas'])
        gt_c = oracle.move_pelvis(T(batch['gt_j3d']))
        dj = torch.randn(B, 17, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        Jt = T(J).double().requires_grad_(True)
        xr, br = x6.double().requires_grad_(True), betas.double().requires_grad_(True)
        R = oracle.rot6d_to_rotmat(xr.reshape(-1, 6)).view(B, 24, 3, 3)
        ref_j, ref_v = oracle.find_joints(oracle.OracleSMPL(model, dtype=torch.float64), br, R[:, :1], R[:, 1:], Jt,
                                          mask=oracle.find_j_reg_mask(Jt.detach()), return_verts=True)
        (ref_j * dj).sum().backward()
        o, p, b_, _ = oracle.refine_poses(oracle.OracleSMPL(model), T(J), x6[:, :1], x6[:, 1:], betas, gt_c, 3)
        _refs[key] = dict(x6=x6, betas=betas, gt_c=gt_c, dj=dj, joints=ref_j.detach(), verts=ref_v.detach(), dx=xr.grad, db=br.grad,
                          dJ=Jt.grad, it_x=torch.cat([o, p], 1), it_b=b_)
    return _refs[key]


def _three_iterations(em, eng, ref, B, mean_bound=5e-6):
    xd, bd = ref['x6'].to(DEV).contiguous(), ref['betas'].to(DEV).contiguous()
    m, v = torch.zeros(B, 154, device=DEV), torch.zeros(B, 154, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    eng.refine_run(xd, bd, ref['gt_c'].to(DEV).contiguous(), m, v, step, 1e-2, 3)
    d = (xd.cpu() - ref['it_x']).abs()
    print('three iterations: pose error max / mean', d.max().item(), d.mean().item(), 'betas', (bd.cpu() - ref['it_b']).abs().max().item())
    assert d.max().item() < 6e-4 and d.mean().item() < mean_bound, (d.max().item(), d.mean().item())
    assert (bd.cpu() - ref['it_b']).abs().max().item() < 3e-4
    return xd.cpu(), bd.cpu()


@pytest.mark.parametrize('B', [128, 130])
@pytest.mark.parametrize('kind', list(BODIES))
def test_lbs_forward_backward_and_three_iterations_vs_oracle(smpl_model_np, j_h36m_np, kind, B):
    model, dm = _body(kind, smpl_model_np)
    em = _mod('engine')
    ref = _reference(model, BODIES[kind][1], j_h36m_np, B)
    eng = em.RefineEngine(dm, B, flags=em.FLAG_KEEP_VERTS)
    assert eng.info['BP'] == (128 if B == 128 else 256), eng.info
    eng.set_j_regressor(T(j_h36m_np))
    xd, bd = ref['x6'].to(DEV).contiguous(), ref['betas'].to(DEV).contiguous()
    djd = ref['dj'].float().to(DEV)
    joints, verts = eng.find_joints_forward(bd, x6d=xd, return_verts=True)
    assert (verts.cpu().double() - ref['verts']).abs().max().item() < 2e-5
    assert (joints.cpu().double() - ref['joints']).abs().max().item() < 2e-5
    # The vertex buffer [3][VP / 4][BP][4] lives in the engine's workspace, padded pose columns and all (B = 130: 126 of them, a whole
    # pose group of padding among them): the same call again leaves every byte of the workspace as it was -- a store that strayed past
    # its row quad or into a padded column's neighbour would show as a difference here or in the vertices above
    torch.cuda.synchronize()
    before = eng.workspace.clone()
    joints2, verts2 = eng.find_joints_forward(bd, x6d=xd, return_verts=True)
    torch.cuda.synchronize()
    assert torch.equal(eng.workspace, before)
    assert torch.equal(joints2, joints) and torch.equal(verts2, verts)
    # the backward reads v_posed as the forward stored it (row quads, global stores from SGPR row bases)
    dx, db, dJ = eng.find_joints_backward(bd, djd, x6d=xd, want_dJ=True)
    errs = (_relerr(dx, ref['dx']), _relerr(db, ref['db']), _relerr(dJ, ref['dJ']))
    print(kind, B, 'relative errors dx6d / dbetas / dJ:', errs)
    assert max(errs) < 2e-4, errs
    assert (dJ.cpu()[T(j_h36m_np) <= 0] == 0).all()
    # three iterations of the loop: k_lbs_fwd<STORE_VP>, k_lbs_bwd16, k_blend_adjoint
    loop = em.RefineEngine(dm, B)
    loop.set_j_regressor(T(j_h36m_np))
    _three_iterations(em, loop, ref, B)


def _wide_support_regressor():
    """17 x 6 = 102 support vertices: more than the per-vertex iteration is built for, so FLAG_SUPPORT_TILES runs the TILE LISTS
    (k_lbs_fwd<.., LIST>, k_lbs_bwd16<.., LIST>, k_blend_adjoint<true>) in every process -- JRR_SUPPORT_FUSED=0, which selects them for
    the shipped regressor too, is read once per process and cannot be set from a test"""
    rng = np.random.RandomState(11)
    J = np.zeros((17, 6890), np.float32)
    cols = rng.choice(6890, 17 * 6, replace=False).reshape(17, 6)
    for i in range(17):
        J[i, cols[i]] = rng.dirichlet(np.ones(6)).astype(np.float32)
    return J


_J102 = _wide_support_regressor()


@pytest.mark.parametrize('B', [128, 130])
def test_listed_tiles_three_iterations_vs_oracle_and_itself(smpl_model_np, B):
    model, dm = _body('slots8', smpl_model_np)
    em = _mod('engine')
    ref = _reference(model, False, _J102, B)
    eng = em.RefineEngine(dm, B, flags=em.FLAG_KEEP_VERTS | em.FLAG_SUPPORT_TILES)
    eng.set_j_regressor(T(_J102))
    assert eng.j_support_info()[1]
    assert eng.support_tiles()[0] == support_tiles_available() and eng.support_vertices() == (False, 0)
    # (the bounds tests/test_gpu_bwd16_waits.py holds the same regressor to)
    runs = [_three_iterations(em, eng, ref, B, mean_bound=1e-5) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
