"""What tests/test_gpu_support_shapes.py and tests/test_gpu_adversarial_gradient.py share: one refine_run iteration from zeroed Adam
moments on an engine, the oracle's gradient of the same state in float64 and float32, and the rule that compares them -- per pose,
e(g) = |g - g64|_2 / |g64|_2 with g_h = adam_m / (1 - beta1), and e(g_h) <= max(3 e(g32), 2e-4); the same for the ten betas entries
alone and, with the floor 1e-5, for the per-pose squared joint error.  The cases are dicts with the keys tests/support_cases.py
builds plus the tensors x6, betas, cam, gt_c, Jt, mt and name, B, body_key."""
import os

import numpy as np
import torch

import oracle
import support_cases as sc
from conftest import support_tiles_available

T = torch.from_numpy
DEV = 'cuda:0'
LR = 1e-2
BETA1_F32 = float(np.float32(1) - np.float32(0.9))     # the kernel's (1 - beta1): m' = (1 - beta1) g from m = 0
G_FLOOR = 2e-4          # tests/test_gpu_parity.py::test_find_joints_backward
SQ_FLOOR = 1e-5         # the rtol of test_joint_loss_and_adam

# ---- bodies and the oracle's results: built once per case, never modified -----------------------------------------------------------
_bodies, _oracles = {}, {}


def _expected_vertices(nsv):
    """what support_vertices() must report: the per-vertex iteration really runs (JRR_SUPPORT_FUSED=0 keeps the tile lists)"""
    on = support_tiles_available() and os.environ.get('JRR_SUPPORT_FUSED') != '0' and nsv <= sc.SUP_NSV
    return (True, nsv) if on else (False, 0)


def _rel_per_pose(a, b):
    a, b = a.double().flatten(1), b.double().flatten(1)
    return (a - b).norm(dim=1) / b.norm(dim=1)


def _body(em, model, key, hint=None):
    """(fp32 oracle SMPL, fp64 oracle SMPL, uploaded body) per body / hint"""
    if key not in _bodies:
        _bodies[key] = (oracle.OracleSMPL(model), oracle.OracleSMPL(model, dtype=torch.float64), em.DeviceModel(model, DEV, hint_vertices=hint))
    return _bodies[key]


def _oracle_grads(c, smpls, sub=slice(None), batch_norm=None, disc=None, gt2d=None, tag='', shape_disc=None):
    """oracle.inner_grad in float64 and float32 on the poses `sub`, and the per-pose squared error of inner_losses' joint term restated
    per pose (with a discriminator: its per-pose sum of (D - 1)^2 as well), in both precisions; memoised"""
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
        ssd = None if shape_disc is None else {k: v.to(dt) for k, v in shape_disc.items()}
        _, gx, gb, gc = oracle.inner_grad(smpl, J, x, b, gt, dsd, ssd, mask=mask, batch_norm=batch_norm, **kw)
        R = oracle.rot6d_to_rotmat(x.reshape(-1, 6)).view(-1, 24, 3, 3)
        joints = oracle.find_joints(smpl, b, R[:, :1], R[:, 1:], J, mask=mask)
        out['g' + name] = torch.cat([gx.flatten(1), gb], 1).double()
        out['gc' + name] = None if gc is None else gc.double()
        out['sq' + name] = ((oracle.move_pelvis(joints) - gt / 1000) ** 2).sum((1, 2)).double()
        if dsd is not None:
            out['D' + name] = oracle.discriminator_forward(dsd, x)[:, :, 0].detach().double()
        if ssd is not None:
            out['S' + name] = oracle.shape_discriminator_forward(ssd, b)[:, 0].detach().double()
    _oracles[key] = out
    return out


def _engine(em, dm, c, per_vertex, disc=None, B=None, shape_disc=None):
    eng = em.RefineEngine(dm, B or c['B'], flags=em.FLAG_KEEP_VERTS | (em.FLAG_SUPPORT_TILES if per_vertex else 0) |
                          (em.FLAG_POSE_DISC if disc is not None else 0) | (em.FLAG_SHAPE_DISC if shape_disc is not None else 0))
    if disc is not None:
        eng.set_pose_disc(em.flatten_state_dict(disc, em.DISC_KEYS))
    if shape_disc is not None:
        eng.set_shape_disc(em.flatten_state_dict(shape_disc, em.SHAPE_DISC_KEYS))
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


def _one_iteration(eng, c, gt2d=None, aux=()):
    """one refine_run iteration from zeroed adam_m / adam_v / step on fresh copies of the case's inputs; aux: 'pose' / 'shape' adds the
    per-pose squared adversarial errors of that iteration (refine_aux_losses) as dsq / ssq"""
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
    if aux:
        dsq, ssq = eng.refine_aux_losses(pose_disc='pose' in aux, shape_disc='shape' in aux)
        out.update({k: t.cpu() for k, t in (('dsq', dsq), ('ssq', ssq)) if t is not None})
    if gt2d is not None:
        eng.set_reprojection(None)
        out.update(cam=cd.cpu(), cam_m=cm.cpu(), cam_v=cv.cpu())
    out.update(x=xd.cpu(), b=bd.cpu(), m=m.cpu(), v=v.cpu(), sq=sq.cpu(), step=int(step.item()))
    return out


def _same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] == b[k]) if k == 'step' else torch.equal(a[k], b[k]), (what, k)


def _check_gradient(r, o, sub, tag, sq_over_batch=False):
    """the rule of the module docstring on one engine's iteration, and the per-pose squared error; prints the case's line of DESIGN.md's table.
    sq_over_batch: the yardstick of the squared error is the fp32 oracle's WORST pose of the batch instead of its error on the same
    pose.  For targets a fraction of a millimetre away the squared error is a difference of nearly equal numbers, fp32 rounding is
    1e-6 .. 8e-5 of it, and one pose's signed error is a single draw that can land near zero (1.3e-6 beside neighbours of 4e-5): three
    times a lucky draw is no bound.  The gradient's yardsticks are norms over 154 and 10 entries and stay per pose."""
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
    assert (s_h <= torch.clamp(3 * (s_32.max() if sq_over_batch else s_32), min=SQ_FLOOR)).all(), (tag, s_h, s_32)


def _synthetic_2d(joints_m, seed, noise=2.0):
    """tests/test_gpu_api.py::_synthetic_2d: the (noisy) joints through a perturbed camera, in the 224-crop pixel frame"""
    gen = torch.Generator().manual_seed(seed)
    B = joints_m.shape[0]
    cam_true = torch.tensor([0.0, 0.0, 2 * 5000 / (224 * 0.9)]).repeat(B, 1) + torch.randn(B, 3, generator=gen) * torch.tensor([0.3, 0.3, 3.0])
    return oracle.project_joints(joints_m, cam_true) + torch.randn(B, 17, 2, generator=gen) * noise


def _targets_2d(c, smpl):
    R = oracle.rot6d_to_rotmat(c['x6'].reshape(-1, 6)).view(-1, 24, 3, 3)
    return _synthetic_2d(oracle.find_joints(smpl, c['betas'], R[:, :1], R[:, 1:], c['Jt'], mask=c['mt']), 2)
