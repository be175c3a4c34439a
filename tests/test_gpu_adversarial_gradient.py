"""The adversarial terms of the inner iteration where a gradient comparison can see them (pytest -m gpu): the inputs of
tests/disc_cases.py -- Gaussian discriminator weights with pose-dependent ReLU masks and outputs in both tails of the sigmoid, targets
a fraction of a millimetre from the start pose so that the discriminator carries 20 .. 100 % of the pose gradient, and poses far from
the rest pose with 6-D columns off the manifold -- through the rule of tests/iteration_checks.py: per pose, the gradient of one
iteration (adam_m / (1 - beta1) from zeroed moments) against oracle.inner_grad in float64 within max(3 x the fp32 oracle's own error,
2e-4), the betas block alone by the same rule, the per-pose squared errors, and every call repeated for bit equality.
tests/test_disc_cases.py pins on the CPU that these inputs expose a discriminator gradient that is 0.2 % too large or one iteration
stale; with the formula weights the suite used before, both pass every bound.

Every case prints `ADV | case | D share | e32 | HIP error | ratio to the bound`.

JRR_SUPPORT_FUSED=2 (the per-vertex iteration as separate launches) is not run here: the library reads that knob once per process, so
it cannot be set for one engine without changing the environment of every other test.
"""
import importlib
import os

import numpy as np
import pytest
import torch

import disc_cases as dc
import oracle
from conftest import PKG_NAME
from iteration_checks import (BETA1_F32, DEV, G_FLOOR, LR, SQ_FLOOR, _body, _check_gradient, _engine, _one_iteration, _oracle_grads,
                              _rel_per_pose, _same_bits, _targets_2d)

pytestmark = pytest.mark.gpu
KNOBS = ('JRR_DENSE_SKINNING', 'JRR_SKIN_JOINTS', 'JRR_VERTEX_ORDER', 'JRR_BWD16')
F32, F64 = torch.float32, torch.float64
BETA1 = float(np.float32(0.9))
OUT_ATOL = 3e-6         # discriminator outputs: tests/test_gpu_parity.py::test_pose_discriminator
DX_RTOL = 5e-4          # its input gradient, of the largest entry
DW_RTOL = 1e-3          # weight gradients per tensor, of the largest entry: tests/test_gpu_api.py::test_pose_disc_weight_gradients


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


def _sub(B):
    """the poses the oracle runs on: all of them up to 64, above that every 32nd with batch_norm = B"""
    return (slice(None), None) if B <= 64 else (slice(3, B, 32), B)


def _oracle(c, model, tag='', gt2d=None):
    """the oracle's gradients and errors on the case (tests/iteration_checks.py::_oracle_grads) and the discriminators' share of the
    float64 gradient per pose: of the pose block with the pose net, of the betas block with the shape net alone"""
    sub, bn = _sub(c['B'])
    o = _oracle_grads(c, dc.smpls(model), sub=sub, batch_norm=bn, disc=c['disc'], shape_disc=c['shape_disc'], gt2d=gt2d, tag='adv' + tag)
    if 'share' not in o:
        if c['disc'] is None and c['shape_disc'] is None:
            o['share'] = torch.zeros(o['g64'].shape[0], dtype=F64)
        else:
            plain = dict(c, disc=None, shape_disc=None, name=c['name'] + '-plain')
            g0 = _oracle_grads(plain, dc.smpls(model), sub=sub, batch_norm=bn, gt2d=gt2d, tag='adv' + tag)['g64']
            cols = slice(0, 144) if c['disc'] is not None else slice(144, 154)
            o['share'] = (o['g64'] - g0)[:, cols].norm(dim=1) / o['g64'][:, cols].norm(dim=1)
    return o, sub


def _line(tag, o, r, sub):
    e_h = _rel_per_pose(r['m'][sub].double() / BETA1_F32, o['g64'])
    e_32 = _rel_per_pose(o['g32'], o['g64'])
    print(f'ADV | {tag} | share {o["share"].min():.3f} .. {o["share"].max():.3f} | e32 {e_32.max():.2e} | HIP {e_h.max():.2e} | '
          f'ratio {(e_h / torch.clamp(3 * e_32, min=G_FLOOR)).max():.3f}')


def _check_aux(r, o, sub, tag):
    """the per-pose squared adversarial errors of the iteration against float64: within 3 x the fp32 oracle's own error or what the
    bound on the outputs themselves (3e-6 each) allows in the sum, sum_k 2 |D_k - 1| 3e-6, whichever is larger"""
    for key, name in (('dsq', 'D'), ('ssq', 'S')):
        if key not in r:
            continue
        n = o[name + '64'].shape[0]
        d64, d32 = (o[name + '64'] - 1).reshape(n, -1), (o[name + '32'] - 1).reshape(n, -1)
        sq64, sq32 = (d64 ** 2).sum(1), (d32 ** 2).sum(1)
        s_h = (r[key][sub].double() - sq64).abs() / sq64
        s_32 = (sq32 - sq64).abs() / sq64
        floor = torch.clamp(2 * OUT_ATOL * d64.abs().sum(1) / sq64, min=SQ_FLOOR)
        print(f'{tag}: {key} {s_h.max():.2e} (fp32 oracle {s_32.max():.2e}, floor {floor.min():.1e} .. {floor.max():.1e})')
        assert (s_h <= torch.maximum(3 * s_32, floor)).all(), (tag, key, s_h, s_32, floor)


def _folded_engine(em, dm, c):
    eng = em.RefineEngine(dm, c['B'], flags=em.FLAG_FOLDED | (em.FLAG_POSE_DISC if c['disc'] is not None else 0))
    eng.set_folded(True)
    eng.set_j_regressor(c['Jt'], c['mt'])
    if c['disc'] is not None:
        eng.set_pose_disc(em.flatten_state_dict(c['disc'], em.DISC_KEYS))
    return eng


def _make_engine(em, dm, c, engine):
    if engine == 'folded':
        return _folded_engine(em, dm, c)
    return _engine(em, dm, c, engine != 'all tiles', disc=c['disc'], shape_disc=c['shape_disc'])


def _run_case(em, model, c, engine, tag, o=None, sub=None, gt2d=None):
    """one iteration on a new engine, the same call again for the same bits, then the rule"""
    if o is None:
        o, sub = _oracle(c, model)
    dm = _body(em, c['model'], c['body_key'])[2]
    aux = tuple(k for k, sd in (('pose', c['disc']), ('shape', c['shape_disc'])) if sd is not None)
    eng = _make_engine(em, dm, c, engine)
    r = _one_iteration(eng, c, gt2d, aux=aux)
    _same_bits(_one_iteration(eng, c, gt2d, aux=aux), r, tag + ', second call')
    _line(tag, o, r, sub)
    _check_gradient(r, o, sub, tag, sq_over_batch=c['kind'] in ('dominant', 'balanced', 'shape'))      # the converged targets
    _check_aux(r, o, sub, tag)
    return r, eng


# ---- B1. one iteration with the strong pose weights ----------------------------------------------------------------------------------
ENGINES = [('per vertex', 64, 'h36m'), ('per vertex', 544, 'h36m'), ('all tiles', 64, 'h36m'), ('tile lists', 64, 'n65'), ('folded', 64, 'h36m')]


@pytest.mark.parametrize('kind', ['dominant', 'balanced'])
@pytest.mark.parametrize('engine,B,support', ENGINES)
def test_one_iteration_strong_pose_disc(em, sm, smpl_model_np, kind, engine, B, support):
    """targets 0.3 mm (the discriminator carries 60 .. 100 % of the pose gradient) and 1.0 mm (22 .. 87 % at B = 64) from the start pose.  Per-vertex
    engine: 64 poses run the pair k_sup_step<1> / <2> beside the GEMMs, 544 the composed k_sup_step<0>, ragged in its 32-pose groups
    (oracle on 17 strided poses, batch_norm = 544); all tiles: k_prep_fwd_dconv / k_dconv_bwd_reduce; a 65-vertex support: the tile
    lists; the folded regressor.  pose_disc_sq per pose as well."""
    c = dc.build(sm, smpl_model_np, kind, B=B, support=support)
    _, eng = _run_case(em, smpl_model_np, c, engine, f'B1 {kind} B = {B} [{engine}]')
    if engine == 'tile lists':
        assert eng.support_vertices() == (False, 0) and eng.support_tiles()[1] < 216


# ---- B2. the H2T hand-over -----------------------------------------------------------------------------------------------------------
def _run_calls(eng, c, calls):
    """refine_run calls of the given lengths on one set of buffers from zeroed moments; the buffers after each call"""
    B = c['B']
    xd, bd, gd = c['x6'].clone().to(DEV), c['betas'].clone().to(DEV), c['gt_c'].to(DEV).contiguous()
    m, v = torch.zeros(B, 154, device=DEV), torch.zeros(B, 154, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    states = []
    for n in calls:
        eng.refine_run(xd, bd, gd, m, v, step, LR, n)
        states.append(dict(x=xd.cpu().clone(), b=bd.cpu().clone(), m=m.cpu().clone(), v=v.cpu().clone(), step=int(step.item())))
    return states


@pytest.mark.parametrize('B', [64, 544])
def test_h2t_hand_over_three_iterations(em, sm, smpl_model_np, B):
    """Three iterations as one call read the per-joint MLP forward that each iteration's k_sup_step leaves in H2T for the next; three
    calls of one recompute it: x6d, betas, adam_m, adam_v and step must be the same bits, and a call of two the same as two calls.
    The third iteration's gradient, g_3 = (m_3 - beta1 m_2) / (1 - beta1), against the float64 oracle at the state the HIP loop reached
    after two iterations, by the rule with e32 at that state.  The differencing costs a few ulps of m: the fp32 oracle's gradients at
    the HIP loop's three states, accumulated into fp32 moments and differenced the same way, give the yardstick e32d, and the bound is
    max(3 e32, 3 e32d, 2e-4).  Measured on the CPU oracle's own trajectory (B = 64), at the state after two iterations: e32 1.0e-6 ..
    4.0e-5, e32d 9.9e-7 .. 4.1e-5 (the differencing costs nothing that shows), the discriminator's share 3 .. 25 % (two Adam steps of
    1e-2 per entry move the joints by centimetres); a discriminator gradient taken at the poses one iteration before is 9.6 .. 180 times
    that bound."""
    c = dc.build(sm, smpl_model_np, 'dominant', B=B)
    dm = _body(em, c['model'], c['body_key'])[2]
    eng = _engine(em, dm, c, True, disc=c['disc'])
    one = _run_calls(eng, c, [3])[0]
    s1, s2, s3 = _run_calls(eng, c, [1, 1, 1])
    _same_bits(one, s3, f'B = {B}: one call of three against three calls of one')
    _same_bits(_run_calls(eng, c, [2])[0], s2, f'B = {B}: one call of two against two calls of one')
    assert s3['step'] == 3
    sub, bn = _sub(B)
    smpls = dc.smpls(smpl_model_np)
    at = lambda s, k: dict(c, x6=s['x'], betas=s['b'], name=f'{c["name"]}-h2t{k}')
    o = _oracle_grads(at(s2, 2), smpls, sub=sub, batch_norm=bn, disc=c['disc'], tag='adv')
    g_h = (s3['m'][sub].double() - BETA1 * s2['m'][sub].double()) / BETA1_F32
    # the fp32 oracle treated the same way
    g32 = [_oracle_grads(cc, smpls, sub=sub, batch_norm=bn, disc=c['disc'], tag='adv')['g32'].float()
           for cc in (c, at(s1, 1))] + [o['g32'].float()]
    m = torch.zeros_like(g32[0])
    moments = []
    for g in g32:
        m = m * np.float32(0.9) + g * np.float32(BETA1_F32)
        moments.append(m.clone())
    g_d = (moments[2].double() - BETA1 * moments[1].double()) / BETA1_F32
    e_h, e_32, e_d = _rel_per_pose(g_h, o['g64']), _rel_per_pose(o['g32'], o['g64']), _rel_per_pose(g_d, o['g64'])
    bound = torch.clamp(3 * torch.maximum(e_32, e_d), min=G_FLOOR)
    g0 = _oracle_grads(dict(at(s2, 2), name=c['name'] + '-h2t2-plain'), smpls, sub=sub, batch_norm=bn, tag='adv')['g64']
    share = (o['g64'] - g0)[:, :144].norm(dim=1) / o['g64'][:, :144].norm(dim=1)
    print(f'ADV | B2 third iteration B = {B} [per vertex] | share {share.min():.3f} .. {share.max():.3f} | e32 {e_32.max():.2e} (differenced {e_d.max():.2e}) | '
          f'HIP {e_h.max():.2e} | ratio {(e_h / bound).max():.3f}')
    assert (e_h <= bound).all(), (e_h, e_32, e_d)


# ---- B3. the shape discriminator -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('engine', ['per vertex', 'all tiles'])
def test_one_iteration_strong_shape_disc(em, sm, smpl_model_np, engine):
    """k_shape_disc and the gb_extra hand-over: strong shape weights, targets 0.3 mm from the start pose, B = 37 (ragged): the shape net
    carries 78 .. 100 % of the betas gradient; the betas block alone by the rule, shape_disc_sq per pose"""
    c = dc.build(sm, smpl_model_np, 'shape', B=37)
    _run_case(em, smpl_model_np, c, engine, f'B3 shape B = 37 [{engine}]')


# ---- B4. the operators at the strong weights -----------------------------------------------------------------------------------------
def _against(got, ref64, ref32, fixed, what, of_max=True):
    """max |got - ref64| (of the largest |ref64| entry when of_max) within max(fixed, 3 x the fp32 oracle's own distance); prints both"""
    scale = ref64.abs().max().clamp_min(1e-30) if of_max else 1.0
    e_h = float((got.detach().cpu().double() - ref64).abs().max() / scale)
    e_32 = float((ref32.double() - ref64).abs().max() / scale)
    print(f'{what}: HIP {e_h:.2e} | fp32 oracle {e_32:.2e} | bound {max(fixed, 3 * e_32):.2e} | ratio {e_h / max(fixed, 3 * e_32):.3f}')
    assert e_h <= max(fixed, 3 * e_32), (what, e_h, e_32)


def _disc_refs(sd, x, gout, B, dtype):
    """outputs, d(10 mean over B x 25 of (D - 1)^2)/dx and the vjp of gout on the poses x, in dtype"""
    sdt = {k: v.to(dtype) for k, v in sd.items()}
    xr = x.to(dtype).clone().requires_grad_(True)
    out = oracle.discriminator_forward(sdt, xr)[:, :, 0]
    gx, = torch.autograd.grad(((out - 1) ** 2).sum() / (B * 25) * 10.0, xr, retain_graph=True)
    gv, = torch.autograd.grad((out * gout.to(dtype)).sum(), xr)
    return out.detach(), gx, gv


@pytest.mark.parametrize('B', [100, 2100])
def test_pose_disc_operators_mixed_masks(em, sm, smpl_model_np, B):
    """pose_disc_forward / pose_disc_backward_input / pose_disc_vjp_input with masks that differ from pose to pose, on a third synthetic
    poses, a third far-batch 6-D values (up to 4 in magnitude) and a third 0.6 randn: B = 100 (ragged), B = 2100 (the 128 x 32 tile
    tier, ragged in its 128-column tiles; the oracle on 33 strided poses)"""
    sd = dc.strong_pose_disc()
    x = dc.operator_inputs(sm, smpl_model_np, dc.shipped_regressor(sm), B, seed=21)
    assert float(x.abs().max()) > 2.5
    idx = torch.arange(B) if B <= 100 else torch.arange(7, B, 64)
    assert len(idx) in (100, 33) and {int(i) % 3 for i in idx} == {0, 1, 2}
    gen = torch.Generator().manual_seed(4)
    gout = torch.randn(B, 25, generator=gen)
    dm = _body(em, smpl_model_np, ('surface', None))[2]
    eng = em.RefineEngine(dm, B, flags=em.FLAG_POSE_DISC)
    eng.set_pose_disc(em.flatten_state_dict(sd, em.DISC_KEYS))
    xd = x.to(DEV)
    out = eng.pose_disc_forward(xd)
    dx = eng.pose_disc_backward_input(xd, 10.0, 1.0)
    out_again = eng.pose_disc_forward(xd)
    dv = eng.pose_disc_vjp_input(xd, gout.to(DEV))
    assert torch.equal(out, out_again)
    o64, gx64, gv64 = _disc_refs(sd, x[idx], gout[idx], B, F64)
    o32, gx32, gv32 = _disc_refs(sd, x[idx], gout[idx], B, F32)
    assert float(o64.min()) < 0.1 and float(o64.max()) > 0.9
    _against(out[idx], o64, o32, OUT_ATOL, f'B4 B = {B} outputs', of_max=False)
    _against(dx[idx], gx64, gx32, DX_RTOL, f'B4 B = {B} backward_input')
    _against(dv[idx], gv64, gv32, DX_RTOL, f'B4 B = {B} vjp_input')


@pytest.mark.parametrize('B', [300, 1100])
def test_pose_disc_weight_gradients_mixed_masks(em, sm, smpl_model_np, B):
    """pose_disc_backward_params (both terms of the discriminator update) with the strong weights on the mixed inputs: B = 300 (two
    pose splits, ragged), B = 1100 (four), against discriminator_update_loss_and_grads on the whole batch"""
    sd = dc.strong_pose_disc()
    J = dc.shipped_regressor(sm)
    xo, xs = dc.operator_inputs(sm, smpl_model_np, J, B, seed=22), dc.operator_inputs(sm, smpl_model_np, J, B, seed=23)
    dm = _body(em, smpl_model_np, ('surface', None))[2]
    eng = em.RefineEngine(dm, B, flags=em.FLAG_POSE_DISC)
    eng.set_pose_disc(em.flatten_state_dict(sd, em.DISC_KEYS))
    dP = torch.zeros(em.DISC_PARAMS, device=DEV)
    l0 = eng.pose_disc_backward_params(xo.to(DEV), 0.0, dP)
    l1 = eng.pose_disc_backward_params(xs.to(DEV), 1.0, dP)
    loss64, ref64 = oracle.discriminator_update_loss_and_grads({k: v.double() for k, v in sd.items()}, xo.double(), xs.double())
    loss32, ref32 = oracle.discriminator_update_loss_and_grads(sd, xo, xs)
    e_l, e_l32 = abs(float((l0 + l1).double().sum()) / (B * 25) - float(loss64)) / float(loss64), abs(float(loss32) - float(loss64)) / float(loss64)
    print(f'B4 B = {B} update loss: HIP {e_l:.2e} | fp32 oracle {e_l32:.2e}')
    assert e_l <= max(1e-5, 3 * e_l32)
    got = em.unflatten_state_dict(dP.cpu(), sd, em.DISC_KEYS)
    for k in em.DISC_KEYS:
        _against(got[k], ref64[k], ref32[k], DW_RTOL, f'B4 B = {B} dW {k}')


# ---- B5. far poses ---------------------------------------------------------------------------------------------------------------------
FAR_B = 33


@pytest.mark.parametrize('engine', ['per vertex', 'all tiles', 'folded'])
def test_far_batch_one_iteration(em, sm, smpl_model_np, engine):
    """the chain (k_prep_fwd, k_chain_bwd, k_sup_step), the pose-blend features R - I, skinning and its adjoints at rotations of 1.2 ..
    2.8 rad, an upside-down root and 6-D columns of norm 0.25 .. 4 at 15 .. 165 degrees to each other; no discriminator.  The fp32
    oracle is within 3.4e-6 of float64 here: the floor decides.  The folded engine by the same rule, and against the dense one within
    the sum of their two bounds."""
    c = dc.build(sm, smpl_model_np, 'far', B=FAR_B)
    r, _ = _run_case(em, smpl_model_np, c, engine, f'B5 far B = {FAR_B} [{engine}]')
    if engine == 'folded':
        dm = _body(em, c['model'], c['body_key'])[2]
        dense = _one_iteration(_engine(em, dm, c, False), c)
        d = _rel_per_pose(r['m'], dense['m'])
        print(f'B5 far: folded against dense, per pose {d.max():.2e}')
        assert (d <= 2 * G_FLOOR).all(), d


@pytest.mark.parametrize('engine', ['per vertex', 'all tiles'])
def test_far_batch_one_iteration_with_2d_term(em, sm, smpl_model_np, engine):
    """the same with the 2-D reprojection term; the camera gradient (cam_m / (1 - beta1)) by the rule, as in
    tests/test_gpu_support_shapes.py::test_one_iteration_with_2d_term"""
    c = dc.build(sm, smpl_model_np, 'far', B=FAR_B)
    gt2d = _targets_2d(c, dc.smpls(smpl_model_np)[0])
    o, sub = _oracle(c, smpl_model_np, tag='2d', gt2d=gt2d)
    tag = f'B5 far + 2-D B = {FAR_B} [{engine}]'
    r, _ = _run_case(em, smpl_model_np, c, engine, tag, o=o, sub=sub, gt2d=gt2d)
    ec_h, ec_32 = _rel_per_pose(r['cam_m'].double() / BETA1_F32, o['gc64']), _rel_per_pose(o['gc32'], o['gc64'])
    print(f'{tag}: camera e(g_h) max {ec_h.max():.2e} | e(g32) max {ec_32.max():.2e}')
    assert (ec_h <= torch.clamp(3 * ec_32, min=G_FLOOR)).all(), (tag, ec_h, ec_32)
    assert (r['cam'] - c['cam']).abs().max().item() > 5e-3                # the camera's Adam ran


def test_far_batch_find_joints_forward_and_backward(em, sm, smpl_model_np):
    """find_joints_forward(return_verts=True) within 2e-5 m of float64, find_joints_backward with x6d and with R inputs within 2e-4 of
    the largest entry (the bounds of tests/test_gpu_parity.py)"""
    c = dc.build(sm, smpl_model_np, 'far', B=FAR_B)
    dm = _body(em, c['model'], c['body_key'])[2]
    smpl64 = dc.smpls(smpl_model_np)[1]
    B = FAR_B
    gen = torch.Generator().manual_seed(3)
    dj = torch.randn(B, 17, 3, generator=gen, dtype=F64)
    bd = c['betas'].to(DEV)
    for use_R in (False, True):
        J = c['Jt'].double().requires_grad_(True)
        b_r = c['betas'].double().requires_grad_(True)
        if use_R:
            leaf = oracle.rot6d_to_rotmat(c['x6'].double().reshape(-1, 6)).view(B, 24, 3, 3).float().double().requires_grad_(True)
            R = leaf
        else:
            leaf = c['x6'].double().requires_grad_(True)
            R = oracle.rot6d_to_rotmat(leaf.reshape(-1, 6)).view(B, 24, 3, 3)
        joints, verts = oracle.find_joints(smpl64, b_r, R[:, :1], R[:, 1:], J, mask=oracle.find_j_reg_mask(J.detach()), return_verts=True)
        (joints * dj).sum().backward()
        eng = em.RefineEngine(dm, B, flags=em.FLAG_KEEP_VERTS)
        eng.set_j_regressor(c['Jt'])
        kw = dict(R=leaf.detach().float().contiguous().to(DEV)) if use_R else dict(x6d=leaf.detach().float().contiguous().to(DEV))
        jh, vh = eng.find_joints_forward(bd, return_verts=True, **kw)
        dv, djm = (vh.cpu().double() - verts.detach()).abs().max().item(), (jh.cpu().double() - joints.detach()).abs().max().item()
        dpose, db, dJ = eng.find_joints_backward(bd, dj.float().to(DEV), want_dJ=True, **kw)
        rel = lambda a, b: ((a.cpu().double() - b).abs().max() / b.abs().max()).item()
        errs = rel(dpose, leaf.grad), rel(db, b_r.grad), rel(dJ, J.grad)
        print(f'B5 far find_joints [{"R" if use_R else "x6d"}]: vertices {dv:.2e} m, joints {djm:.2e} m, d pose {errs[0]:.2e}, d betas {errs[1]:.2e}, dJ {errs[2]:.2e}')
        assert dv < 2e-5 and djm < 2e-5
        assert max(errs) < 2e-4, errs


def test_far_batch_three_iterations_vs_oracle(em, sm, smpl_model_np):
    """three iterations against the fp32 oracle at the bounds of tests/test_gpu_support_shapes.py::test_three_iterations_vs_oracle: pose
    max < 6e-4, mean < 1e-5, betas < 3e-4.  (The two oracles themselves: max 4.9e-4 -- one entry whose gradient of 2e-8 sits next to
    Adam's eps -- mean 1.4e-7, betas 2.5e-7: tests/test_disc_cases.py.)"""
    c = dc.build(sm, smpl_model_np, 'far', B=FAR_B)
    dm = _body(em, c['model'], c['body_key'])[2]
    o, p, b, _ = oracle.refine_poses(dc.smpls(smpl_model_np)[0], c['Jt'], c['x6'][:, :1], c['x6'][:, 1:], c['betas'], c['gt_c'], 3)
    for engine in ('per vertex', 'all tiles'):
        s = _run_calls(_engine(em, dm, c, engine == 'per vertex'), c, [3])[0]
        d = (s['x'] - torch.cat([o, p], 1)).abs()
        db = (s['b'] - b).abs().max().item()
        print(f'B5 far three iterations [{engine}]: pose max {d.max():.2e} mean {d.mean():.2e} betas {db:.2e}')
        assert d.max().item() < 6e-4 and d.mean().item() < 1e-5, (d.max().item(), d.mean().item())
        assert db < 3e-4, db
        assert s['step'] == 3


@pytest.mark.parametrize('engine', ['per vertex', 'all tiles'])
def test_far_batch_one_iteration_strong_pose_disc(em, sm, smpl_model_np, engine):
    """the strong pose weights on the far batch with its own targets: inputs of up to 4 in magnitude saturate the sigmoid (outputs
    1.5e-11 .. 1 - 1.5e-8) and switch 91 .. 96 % of the units; the joint term dominates (share 0.1 .. 1 %), so this case is about
    finite, repeatable results and pose_disc_sq at large activations"""
    c = dc.build(sm, smpl_model_np, 'far_disc', B=FAR_B)
    _run_case(em, smpl_model_np, c, engine, f'B5 far + pose-D B = {FAR_B} [{engine}]')
