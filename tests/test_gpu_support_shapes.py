"""The per-vertex iteration (csrc/supk.h sup_body, k_sup_gather in csrc/sup.hip, jrr_j_support_info) on the support structures of
tests/support_cases.py (pytest -m gpu): 2 .. 64 support vertices, vertices read by all 17 rows, full and half-empty mask words, the first
vertex and the partial last tile, 1 / 2 / 3 / 6 skinning influences, a joint list at its capacity of 64, a mask, the vertex-order hint,
B = 1, the 64 -> 65 switch to the tile lists, a support that shrinks under in-loop J steps, and re-gathering on one engine.

What is compared is the GRADIENT of one iteration, not poses after Adam steps (Adam's first step is lr g / (|g| + eps): it barely sees
an error in the gradient's magnitude): one refine_run iteration from zeroed moments leaves adam_m = (1 - beta1) g
(tests/test_gpu_loop_length.py), so g_h = adam_m / BETA1_F32, against oracle.inner_grad in float64 (g64), with the float32 oracle (g32) as
the yardstick: per pose, e(g) = |g - g64|_2 / |g64|_2 and e(g_h) <= max(3 e(g32), 2e-4) -- 3 x the fp32 oracle is the margin of
test_gpu_loop_length.py, 2e-4 the bound of test_gpu_parity.py::test_find_joints_backward.  The same holds for an engine WITHOUT
FLAG_SUPPORT_TILES (all 216 tiles through k_lbs_fwd / k_lbs_bwd16 / k_blend_adjoint) on the same inputs: a failure of the per-vertex
engine alone is a bug of the per-vertex path.
"""
import importlib
import os

import numpy as np
import pytest
import torch

import oracle
import support_cases as sc
from conftest import PKG_NAME
from iteration_checks import (DEV, LR, T, _announce, _body, _check_gradient, _engine, _expected_vertices, _one_iteration, _oracle_grads,
                              _rel_per_pose, _same_bits, _targets_2d, BETA1_F32, G_FLOOR)

pytestmark = pytest.mark.gpu
KNOBS = ('JRR_DENSE_SKINNING', 'JRR_SKIN_JOINTS', 'JRR_VERTEX_ORDER', 'JRR_BWD16')


@pytest.fixture(autouse=True)
def _default_kernels_only():
    if any(k in os.environ for k in KNOBS):
        pytest.skip('the suite itself runs under a forced kernel variant')


@pytest.fixture(scope='module')
def em():
    return importlib.import_module(PKG_NAME + '.engine')


@pytest.fixture(scope='module')
def sm():
    return importlib.import_module(PKG_NAME + '.smpl_model')


# ---- inputs and a fresh engine's results: built once per case, never modified (tests/iteration_checks.py keeps bodies and oracles) ----
_cases, _fresh = {}, {}


def _case(sm, smpl_model_np, case, B=None, J=None):
    """the case's regressor and a seeded batch for it; `J`: another regressor on the surface body (the shipped one, the shrinking one)"""
    key = (case, B)
    if key not in _cases:
        if J is None:
            c = sc.build(smpl_model_np, case)
        else:
            c = dict(model=smpl_model_np, body='surface', J=J, mask=None, hint=None, B=sc.B_DEFAULT,
                     support=np.nonzero((J > 0).any(0))[0])
        c['B'] = B or c['B']
        batch = sm.synthetic_batch(c['model'], sc.effective(c['J'], c['mask']), c['B'], seed=sc.BATCH_SEED)
        c['x6'], c['betas'], c['cam'] = T(batch['pose6d']), T(batch['betas']), T(batch['cam'])
        c['gt_c'] = oracle.move_pelvis(T(batch['gt_j3d']))
        c['Jt'] = T(c['J'])
        c['mt'] = None if c['mask'] is None else T(c['mask'])
        c['body_key'] = (c['body'], case if c['hint'] is not None else None)
        c['name'] = case
        _cases[key] = c
    return _cases[key]




def _fresh_result(em, sm, smpl_model_np, case, J=None):
    """one iteration of a FRESH per-vertex engine on the case (3a's run, and the yardstick of 3e); memoised"""
    if case not in _fresh:
        c = _case(sm, smpl_model_np, case, J=J)
        dm = _body(em, c['model'], c['body_key'], c['hint'])[2]
        _fresh[case] = _one_iteration(_engine(em, dm, c, True), c)
    return _fresh[case]


# ---- 3a. gradient and forward of one iteration, every case ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(sc.SPEC))
def test_one_iteration_gradient(em, sm, smpl_model_np, case):
    """per-vertex engine (n65: the tile lists) and all-tiles engine against the fp64 oracle, per pose: the gradient by the rule of the
    module docstring, the per-pose squared error within max(3 x the fp32 oracle's own error, 1e-5) relative; the same call from the same
    start state a second time gives the same bits"""
    c = _case(sm, smpl_model_np, case)
    smpl, smpl64, dm = _body(em, c['model'], c['body_key'], c['hint'])
    if c['hint'] is not None:
        assert dm.info['hinted_vertices_stored_first'] == len(c['support']), dm.info
    if c['body'] == 'influences':
        print(f'{case}: the body with 1 / 2 / 3 / 4 / 6 influences uploads as {dm.info}')
    o = _oracle_grads(c, (smpl, smpl64))
    r_sup = _fresh_result(em, sm, smpl_model_np, case)
    eng = _engine(em, dm, c, True)
    _same_bits(_one_iteration(eng, c), r_sup, 'another engine, same start state')
    _same_bits(_one_iteration(eng, c), r_sup, 'same engine, second call')
    eng_all = _engine(em, dm, c, False)
    r_all = _one_iteration(eng_all, c)
    _same_bits(_one_iteration(eng_all, c), r_all, 'all tiles, second call')
    for tag, r in (('all tiles', r_all), ('tile lists' if case == 'n65' else 'per vertex', r_sup)):      # (the reference engine first)
        _check_gradient(r, o, slice(None), f'{case} [{tag}]')


# ---- 3b. three iterations ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['n64_dense', 'influences', 'one_joint'])
def test_three_iterations_vs_oracle(em, sm, smpl_model_np, case):
    """the bounds tests/test_gpu_round4.py holds this path to: pose max < 6e-4, mean < 1e-5, betas < 3e-4; step == 3 (the last-arriver
    ticket of k_sup_step)"""
    c = _case(sm, smpl_model_np, case)
    smpl, _, dm = _body(em, c['model'], c['body_key'], c['hint'])
    o, p, b, _ = oracle.refine_poses(smpl, c['Jt'], c['x6'][:, :1], c['x6'][:, 1:], c['betas'], c['gt_c'], 3, mask=c['mt'])
    eng = _engine(em, dm, c, True)
    B = c['B']
    xd, bd = c['x6'].clone().to(DEV), c['betas'].clone().to(DEV)
    m, v = torch.zeros(B, 154, device=DEV), torch.zeros(B, 154, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    eng.refine_run(xd, bd, c['gt_c'].to(DEV).contiguous(), m, v, step, LR, 3)
    d = (xd.cpu() - torch.cat([o, p], 1)).abs()
    db = (bd.cpu() - b).abs().max().item()
    print(f'{case}: three iterations: pose max {d.max():.2e} mean {d.mean():.2e} betas {db:.2e}')
    assert d.max().item() < 6e-4 and d.mean().item() < 1e-5, (d.max().item(), d.mean().item())
    assert db < 3e-4, db
    assert int(step.item()) == 3


# ---- 3c. with the other terms ------------------------------------------------------------------------------------------------------
def test_one_iteration_with_2d_term(em, sm, smpl_model_np):
    """n64_dense with the 2-D reprojection term (scripts/optimize.py:231-233): pose + betas gradient and the camera gradient
    (cam_m / BETA1_F32) by the rule of 3a, both with the floor 2e-4, on both engines"""
    c = _case(sm, smpl_model_np, 'n64_dense')
    smpl, smpl64, dm = _body(em, c['model'], c['body_key'])
    gt2d = _targets_2d(c, smpl)
    o = _oracle_grads(c, (smpl, smpl64), gt2d=gt2d, tag='2d')
    ec_32 = _rel_per_pose(o['gc32'], o['gc64'])
    for per_vertex in (False, True):
        tag = 'n64_dense + 2-D [' + ('per vertex' if per_vertex else 'all tiles') + ']'
        eng = _engine(em, dm, c, per_vertex)
        r = _one_iteration(eng, c, gt2d)
        if per_vertex:
            assert eng.support_vertices() == _expected_vertices(64)          # the 2-D term does not leave the per-vertex iteration
        _same_bits(_one_iteration(eng, c, gt2d), r, tag + ', second call')
        _check_gradient(r, o, slice(None), tag)
        ec_h = _rel_per_pose(r['cam_m'].double() / BETA1_F32, o['gc64'])
        print(f'{tag}: camera e(g_h) max {ec_h.max():.2e} | e(g32) max {ec_32.max():.2e}')
        # the fp32 oracle's own camera error here, measured on the CPU: 3.4e-8 .. 2.2e-6 per pose (|gc64| 0.033 .. 0.56): the floor decides
        assert (ec_h <= torch.clamp(3 * ec_32, min=G_FLOOR)).all(), (tag, ec_h, ec_32)
        assert (r['cam'] - c['cam']).abs().max().item() > 5e-3                # the camera's Adam ran


@pytest.mark.parametrize('B', [64, 544])
def test_one_iteration_with_pose_disc(em, sm, smpl_model_np, B):
    """n33_dense with the pose discriminator: B = 64 runs the two-launch form beside the GEMMs (k_sup_step<1> / <2>), B = 544 the composed
    k_sup_step<0> with the MLP adjoint inside sup_body; at 544 the oracle runs on 17 strided poses with batch_norm = 544"""
    c = _case(sm, smpl_model_np, 'n33_dense', B=B)
    smpl, smpl64, dm = _body(em, c['model'], c['body_key'])
    dsd = oracle.formula_state_dict(oracle.DISC_PARAM_SHAPES, seed=0)
    sub, bn = (slice(None), None) if B == 64 else (slice(3, 544, 32), 544)
    o = _oracle_grads(c, (smpl, smpl64), sub=sub, batch_norm=bn, disc=dsd, tag='disc')
    for per_vertex in (False, True):
        tag = f'n33_dense + pose-D, B = {B} [' + ('per vertex' if per_vertex else 'all tiles') + ']'
        eng = _engine(em, dm, c, per_vertex, disc=dsd)
        r = _one_iteration(eng, c)
        _same_bits(_one_iteration(eng, c), r, tag + ', second call')
        _check_gradient(r, o, sub, tag)


# ---- 3d. a shrinking support ---------------------------------------------------------------------------------------------------------
def test_shrinking_support_under_j_steps(em, sm, smpl_model_np):
    """six iterations with a J step after each on a regressor whose weak entries die (200 -> 172 positive entries at B = 33, all 64
    vertices stay): the per-vertex engine reads Jn_vi live over tables gathered for the initial support.  Per-vertex engine, all-tiles
    engine and the oracle loop: the same entries moved and died, |J - J_oracle| < 2e-5, poses within the three-iteration bounds"""
    J0 = sc.shrinking_case()
    c = _case(sm, smpl_model_np, 'shrinking', J=J0)
    dm = _body(em, c['model'], c['body_key'])[2]
    ref = sc.shrinking_oracle(smpl_model_np, J0, c['B'], sm)
    assert torch.equal(ref['x6d'], c['x6']) and torch.equal(ref['gt_c'], c['gt_c'])
    assert min(ref['margin']) > 4e-5                     # which entries die does not hang on rounding (tests/test_support_cases.py)
    J0t = T(J0)
    B = c['B']
    for per_vertex in (True, False):
        tag = 'per vertex' if per_vertex else 'all tiles'
        J = J0t.clone().to(DEV)
        eng = em.RefineEngine(dm, B, flags=em.FLAG_KEEP_VERTS | (em.FLAG_SUPPORT_TILES if per_vertex else 0))
        eng.set_j_regressor(J)
        assert eng.j_support_info()[1]
        if per_vertex:
            assert eng.support_vertices() == _expected_vertices(64)
        Jm, Jv, Js = torch.zeros_like(J), torch.zeros_like(J), torch.zeros(1, dtype=torch.int32, device=DEV)
        xd, bd = c['x6'].clone().to(DEV), c['betas'].clone().to(DEV)
        m, v = torch.zeros(B, 154, device=DEV), torch.zeros(B, 154, device=DEV)
        step = torch.zeros(1, dtype=torch.int32, device=DEV)
        eng.refine_run_j_steps(xd, bd, c['gt_c'].to(DEV).contiguous(), m, v, step, LR, sc.SHRINK_ITERS, 1, J, Jm, Jv, Js, sc.SHRINK_J_LR)
        assert int(Js.item()) == sc.SHRINK_ITERS == int(step.item())
        Jh = J.cpu()
        dJ = (Jh - ref['J']).abs().max().item()
        d = (xd.cpu() - ref['x']).abs()
        db = (bd.cpu() - ref['b']).abs().max().item()
        print(f'shrinking [{tag}]: {int((J0t > 0).sum())} -> {int((Jh > 0).sum())} positive entries, |J - J_oracle| {dJ:.2e}, pose max {d.max():.2e} '
              f'mean {d.mean():.2e} betas {db:.2e}')
        assert torch.equal(Jh != J0t, ref['J'] != J0t) and int((Jh != J0t).sum()) == int((J0t > 0).sum())      # exactly the positive entries moved
        assert torch.equal(Jh > 0, ref['J'] > 0) and int((J0t > 0).sum()) - int((Jh > 0).sum()) >= 10       # the same entries died
        assert dJ < 2e-5, dJ
        assert d.max().item() < 6e-4 and d.mean().item() < 1e-5, (d.max().item(), d.mean().item())
        assert db < 3e-4, db
        if per_vertex:
            assert eng.support_vertices() == _expected_vertices(64)          # still, after the J steps
        counts, fits = eng.j_support_info()                                   # raises on a sticky error word
        assert fits and counts == [int(n) for n in (ref['J'] > 0).sum(1)]
        if per_vertex:
            assert eng.support_vertices() == _expected_vertices(64)          # every vertex is still in some row


# ---- 3e. re-gathering on one engine --------------------------------------------------------------------------------------------------
def test_regather_on_one_engine(em, sm, smpl_model_np, j_h36m_np):
    """one engine takes n64_dense, n2_blocks, the shipped H36M regressor and n64_dense again, each announced with set_j_regressor +
    j_support_info (the tables are gathered over the previous support's): every one-iteration result equals a fresh engine's bit for bit"""
    eng = None
    for case in ('n64_dense', 'n2_blocks', 'h36m', 'n64_dense'):
        J = j_h36m_np if case == 'h36m' else None
        want = _fresh_result(em, sm, smpl_model_np, case, J=J)
        c = _case(sm, smpl_model_np, case, J=J)
        if eng is None:
            eng = _engine(em, _body(em, c['model'], c['body_key'])[2], c, True)
        else:
            _announce(eng, c, True)
        _same_bits(_one_iteration(eng, c), want, f're-gathered for {case}')
