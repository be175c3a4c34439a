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
from conftest import PKG_NAME, support_tiles_available

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
LR = 1e-2
BETA1_F32 = float(np.float32(1) - np.float32(0.9))     # the kernel's (1 - beta1): m' = (1 - beta1) g from m = 0
KNOBS = ('JRR_DENSE_SKINNING', 'JRR_SKIN_JOINTS', 'JRR_VERTEX_ORDER', 'JRR_BWD16')
G_FLOOR = 2e-4          # tests/test_gpu_parity.py::test_find_joints_backward
SQ_FLOOR = 1e-5         # the rtol of test_joint_loss_and_adam


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


def _expected_vertices(nsv):
    """what support_vertices() must report: the per-vertex iteration really runs (JRR_SUPPORT_FUSED=0 keeps the tile lists)"""
    on = support_tiles_available() and os.environ.get('JRR_SUPPORT_FUSED') != '0' and nsv <= sc.SUP_NSV
    return (True, nsv) if on else (False, 0)


def _rel_per_pose(a, b):
    a, b = a.double().flatten(1), b.double().flatten(1)
    return (a - b).norm(dim=1) / b.norm(dim=1)


# ---- bodies, inputs and the oracle's results: built once per case, never modified ----------------------------------------------------
_bodies, _cases, _oracles, _fresh = {}, {}, {}, {}


def _body(em, model, key, hint=None):
    """(fp32 oracle SMPL, fp64 oracle SMPL, uploaded body) per body / hint"""
    if key not in _bodies:
        _bodies[key] = (oracle.OracleSMPL(model), oracle.OracleSMPL(model, dtype=torch.float64), em.DeviceModel(model, DEV, hint_vertices=hint))
    return _bodies[key]


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


def _oracle_grads(c, smpls, sub=slice(None), batch_norm=None, disc=None, gt2d=None, tag=''):
    """oracle.inner_grad in float64 and float32 on the poses `sub`, and the per-pose squared error of inner_losses' joint term restated
    per pose, in both precisions; memoised"""
    key = (c['name'], c['B'], tag)
    if key in _oracles:
        return _oracles[key]
    out = {}
    for smpl, dt, name in ((smpls[1], torch.float64, '64'), (smpls[0], torch.float32, '32')):
        J = c['Jt'].to(dt)
        mask = None if c['mt'] is None else c['mt'].to(dt)
        x, b, gt = c['x6'][sub].to(dt), c['betas'][sub].to(dt), c['gt_c'][sub].to(dt)
        dsd = None if disc is None else {k: v.to(dt) for k, v in disc.items()}
        kw = {} if gt2d is None else dict(gt_j2d=gt2d[sub].to(dt), cam=c['cam'][sub].to(dt))
        _, gx, gb, gc = oracle.inner_grad(smpl, J, x, b, gt, dsd, mask=mask, batch_norm=batch_norm, **kw)
        R = oracle.rot6d_to_rotmat(x.reshape(-1, 6)).view(-1, 24, 3, 3)
        joints = oracle.find_joints(smpl, b, R[:, :1], R[:, 1:], J, mask=mask)
        out['g' + name] = torch.cat([gx.flatten(1), gb], 1).double()
        out['gc' + name] = None if gc is None else gc.double()
        out['sq' + name] = ((oracle.move_pelvis(joints) - gt / 1000) ** 2).sum((1, 2)).double()
    _oracles[key] = out
    return out


def _engine(em, dm, c, per_vertex, disc=None, B=None):
    eng = em.RefineEngine(dm, B or c['B'], flags=em.FLAG_KEEP_VERTS | (em.FLAG_SUPPORT_TILES if per_vertex else 0) |
                          (em.FLAG_POSE_DISC if disc is not None else 0))
    if disc is not None:
        eng.set_pose_disc(em.flatten_state_dict(disc, em.DISC_KEYS))
    _announce(eng, c, per_vertex)
    return eng


def _announce(eng, c, per_vertex):
    """set_j_regressor + j_support_info, and which iteration the engine then runs"""
    eng.set_j_regressor(c['Jt'], c['mt'])
    counts, fits = eng.j_support_info()
    assert fits and counts == [int(n) for n in (sc.effective(c['J'], c['mask']) > 0).sum(1)]
    nsv = len(c['support'])
    if per_vertex:
        assert eng.support_vertices() == _expected_vertices(nsv), (c['name'], eng.support_vertices())
        assert eng.support_tiles()[0] == support_tiles_available()
        if nsv > sc.SUP_NSV:
            assert eng.support_vertices() == (False, 0)          # the tile lists
    else:
        assert eng.support_vertices() == (False, 0) and eng.support_tiles() == (False, 216)


def _one_iteration(eng, c, gt2d=None):
    """one refine_run iteration from zeroed adam_m / adam_v / step on fresh copies of the case's inputs"""
    B = c['B']
    xd, bd, gd = c['x6'].clone().to(DEV), c['betas'].clone().to(DEV), c['gt_c'].to(DEV).contiguous()
    m, v = torch.zeros(B, 154, device=DEV), torch.zeros(B, 154, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    sq = torch.zeros(B, device=DEV)
    out = {}
    if gt2d is not None:
        cd, cm, cv = c['cam'].clone().to(DEV), torch.zeros(B, 3, device=DEV), torch.zeros(B, 3, device=DEV)
        eng.set_reprojection(gt2d.to(DEV).contiguous(), cd, cm, cv)
    eng.refine_run(xd, bd, gd, m, v, step, LR, 1, sqerr=sq)
    if gt2d is not None:
        eng.set_reprojection(None)
        out.update(cam=cd.cpu(), cam_m=cm.cpu(), cam_v=cv.cpu())
    out.update(x=xd.cpu(), b=bd.cpu(), m=m.cpu(), v=v.cpu(), sq=sq.cpu(), step=int(step.item()))
    return out


def _same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] == b[k]) if k == 'step' else torch.equal(a[k], b[k]), (what, k)


def _check_gradient(r, o, sub, tag):
    """the rule of the module docstring on one engine's iteration, and the per-pose squared error; prints the case's line of DESIGN.md's table"""
    g_h = r['m'][sub].double() / BETA1_F32
    e_h, e_32 = _rel_per_pose(g_h, o['g64']), _rel_per_pose(o['g32'], o['g64'])
    s_h = (r['sq'][sub].double() - o['sq64']).abs() / o['sq64']
    s_32 = (o['sq32'] - o['sq64']).abs() / o['sq64']
    print(f'{tag}: e(g_h) max {e_h.max():.2e} | e(g32) max {e_32.max():.2e} | ratio to the bound '
          f'{(e_h / torch.clamp(3 * e_32, min=G_FLOOR)).max():.3f} | sqerr {s_h.max():.2e} (fp32 oracle {s_32.max():.2e}) | '
          f'|g64| {o["g64"].norm(dim=1).min():.2e} .. {o["g64"].norm(dim=1).max():.2e}')
    # The ten betas entries alone, by the same rule.  Most of the pose gradient's norm arrives through dA (the skinning transforms); the
    # betas read the vertices through the blend basis as well (dF = Ds^T dvp): an error of that product alone is diluted some ten times
    # in the norm over all 154 entries (dF scaled by 1.002: 1.0e-4 .. 3.9e-4 there).
    eb_h, eb_32 = _rel_per_pose(g_h[:, 144:], o['g64'][:, 144:]), _rel_per_pose(o['g32'][:, 144:], o['g64'][:, 144:])
    print(f'{tag}: betas alone e(g_h) max {eb_h.max():.2e} | e(g32) max {eb_32.max():.2e}')
    assert r['step'] == 1
    assert torch.isfinite(r['m']).all() and torch.isfinite(r['x']).all()
    assert (e_h <= torch.clamp(3 * e_32, min=G_FLOOR)).all(), (tag, e_h, e_32)
    assert (eb_h <= torch.clamp(3 * eb_32, min=G_FLOOR)).all(), (tag, eb_h, eb_32)
    assert (s_h <= torch.clamp(3 * s_32, min=SQ_FLOOR)).all(), (tag, s_h, s_32)


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
def _synthetic_2d(joints_m, seed, noise=2.0):
    """tests/test_gpu_api.py::_synthetic_2d: the (noisy) joints through a perturbed camera, in the 224-crop pixel frame"""
    gen = torch.Generator().manual_seed(seed)
    B = joints_m.shape[0]
    cam_true = torch.tensor([0.0, 0.0, 2 * 5000 / (224 * 0.9)]).repeat(B, 1) + torch.randn(B, 3, generator=gen) * torch.tensor([0.3, 0.3, 3.0])
    return oracle.project_joints(joints_m, cam_true) + torch.randn(B, 17, 2, generator=gen) * noise


def _targets_2d(c, smpl):
    R = oracle.rot6d_to_rotmat(c['x6'].reshape(-1, 6)).view(-1, 24, 3, 3)
    return _synthetic_2d(oracle.find_joints(smpl, c['betas'], R[:, :1], R[:, 1:], c['Jt'], mask=c['mt']), 2)


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
