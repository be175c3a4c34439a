"""Inputs under which the adversarial terms of the inner iteration are VISIBLE to a gradient comparison: seeded builders, and the
measurements that tests/test_disc_cases.py pins on the CPU oracle and tests/test_gpu_adversarial_gradient.py relies on.  No GPU.

What the suite drove the discriminator code with before: oracle.formula_state_dict weights (a sinusoid of the flat index: every matrix
has rank 2, D's outputs stay in 0.48 .. 0.53, 3 % of the fc0 and 0.1 % of the fc2 units change with the pose) on synthetic_batch poses
(every joint within N(0, 0.3^2) of the rest pose, unit-length orthogonal 6-D columns) with targets 10 mm of noise away, where the
discriminator contributes 1e-5 .. 1e-4 of the pose gradient -- below every bound an iteration-level test holds.  Here:

  strong_pose_disc / strong_shape_disc   Gaussian weights of full rank whose ReLU masks differ from pose to pose and whose outputs
                                         reach both tails of the sigmoid
  converged_targets                      targets a fraction of a millimetre from the start pose's own joints, as late in the loop: the
                                         joint term is small and the discriminator carries most of the gradient
  far_batch                              poses far from the rest pose (a flipped root, limbs bent by 1.2 .. 2.8 rad) whose 6-D columns
                                         are neither unit length nor orthogonal
  operator_inputs                        a third synthetic poses, a third far_batch 6-D values, a third 0.6 randn
"""
import numpy as np
import torch

import oracle
import support_cases as sc

T = torch.from_numpy
NJ = 24
POSE_SEED, SHAPE_SEED = 7, 16
HIDDEN_GAIN, OUT_GAIN, BIAS_GAIN = 1.4, 4.0, 0.1                     # pose net
# shape net (10 -> 10 -> 5 -> 1 on betas ~ N(0, 1)): an output gain of 4 saturates the sigmoid at 1, the target, where the term's
# gradient vanishes (share 1e-10 for some poses); 1.5 at seed 16 gives outputs 0.023 .. 0.943 and a share >= 0.78 for every pose
SHAPE_HIDDEN_GAIN, SHAPE_OUT_GAIN, SHAPE_BIAS_GAIN = 1.4, 1.5, 0.3
BENT = (1, 2, 4, 5, 16, 17, 18, 19)                                  # hips, knees, shoulders, elbows
B_CASE = 64
NOISE_DOMINANT, NOISE_BALANCED = 0.3, 1.0                            # mm
G_FLOOR = 2e-4                                                       # tests/test_gpu_support_shapes.py


# ---- weights -------------------------------------------------------------------------------------------------------------------------
def _gaussian_state_dict(shapes, seed, hidden, out, bias, out_rows):
    rng = np.random.RandomState(seed)
    sd = {}
    for name, shp in shapes:
        w = rng.standard_normal(shp)
        if name.endswith('bias'):
            w = bias * w
        else:
            w = (out if name in out_rows else hidden) * w / np.sqrt(np.prod(shp[1:]))
        sd[name] = T(w.astype(np.float32))
    return sd


def strong_pose_disc(seed: int = POSE_SEED):
    """hidden weights 1.4 randn / sqrt(fan_in), the 25 output rows 4 randn / sqrt(fan_in), biases 0.1 randn; float32, in
    oracle.DISC_PARAM_SHAPES order"""
    out_rows = {f'linears.{i}.weight' for i in range(NJ)} | {'linear_operations.4.weight'}
    return _gaussian_state_dict(oracle.DISC_PARAM_SHAPES, seed, HIDDEN_GAIN, OUT_GAIN, BIAS_GAIN, out_rows)


def strong_shape_disc(seed: int = SHAPE_SEED):
    return _gaussian_state_dict(oracle.SHAPE_DISC_PARAM_SHAPES, seed, SHAPE_HIDDEN_GAIN, SHAPE_OUT_GAIN, SHAPE_BIAS_GAIN,
                                {'shape_operations.4.weight'})


def weight_matrices(sd):
    """every weight tensor as a 2-D matrix (rows = outputs); the 24 per-joint rows stacked into one (24, 32) matrix"""
    out = {k: v.double().flatten(1) for k, v in sd.items() if k.endswith('weight') and not k.startswith('linears.')}
    heads = [sd[k].double().flatten() for k in sd if k.startswith('linears.') and k.endswith('weight')]
    if heads:
        out['linears.*.weight'] = torch.stack(heads)
    return out


def pose_disc_activity(sd, x6d):
    """float64 forward of oracle.discriminator_forward that keeps the pre-activations: per hidden layer the share of units that are on
    for some poses of the batch and off for others (conv layers: a unit is a (joint, channel) pair), and the outputs (B, 25)"""
    sd = {k: v.double() for k, v in sd.items()}
    x = x6d.double()                                                           # (B, 24, 6)
    pre = {}
    pre['conv0'] = x @ sd['conv_operations.0.weight'].flatten(1).T + sd['conv_operations.0.bias']
    h = torch.relu(pre['conv0'])
    pre['conv2'] = h @ sd['conv_operations.2.weight'].flatten(1).T + sd['conv_operations.2.bias']
    conv = torch.relu(pre['conv2'])                                            # (B, 24, 32): flatten index = joint * 32 + channel
    pre['fc0'] = conv.flatten(1) @ sd['linear_operations.0.weight'].T + sd['linear_operations.0.bias']
    pre['fc2'] = torch.relu(pre['fc0']) @ sd['linear_operations.2.weight'].T + sd['linear_operations.2.bias']
    mixed = {}
    for k, p in pre.items():
        on = (p > 0).flatten(1)
        mixed[k] = float((on.any(0) & ~on.all(0)).double().mean())
    out = oracle.discriminator_forward(sd, x)[:, :, 0]
    return mixed, out


def shape_disc_activity(sd, betas):
    sd = {k: v.double() for k, v in sd.items()}
    p0 = betas.double() @ sd['shape_operations.0.weight'].T + sd['shape_operations.0.bias']
    p2 = torch.relu(p0) @ sd['shape_operations.2.weight'].T + sd['shape_operations.2.bias']
    mixed = {k: float(((p > 0).any(0) & ~(p > 0).all(0)).double().mean()) for k, p in (('fc0', p0), ('fc2', p2))}
    return mixed, oracle.shape_discriminator_forward(sd, betas.double())[:, 0]


# ---- targets and poses ---------------------------------------------------------------------------------------------------------------
def _joints64_mm(model, J, x6d, betas):
    """float64 pelvis-centred joints of the poses, in mm"""
    smpl = oracle.OracleSMPL(model, dtype=torch.float64)
    R = oracle.rot6d_to_rotmat(T(np.asarray(x6d)).double().reshape(-1, 6)).view(-1, NJ, 3, 3)
    j = oracle.find_joints(smpl, T(np.asarray(betas)).double(), R[:, :1], R[:, 1:], T(np.asarray(J)).double())
    return oracle.move_pelvis(j).numpy() * 1000.0


def converged_targets(model, J, batch, noise_mm: float, seed: int = 0) -> np.ndarray:
    """gt_j3d (B, 17, 3) float32, mm: the float64 joints of the batch's own start pose, pelvis-centred, plus N(0, noise_mm^2),
    re-centred -- the joint term as small as it is late in the loop"""
    rng = np.random.RandomState(seed)
    gt = _joints64_mm(model, J, batch['pose6d'], batch['betas'])
    gt = gt + rng.normal(0.0, noise_mm, size=gt.shape)
    return (gt - gt[:, :1]).astype(np.float32)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def far_batch(model, J, B: int, seed: int = 0, targets: bool = True):
    """The keys of synthetic_batch.  Global orientation: a rotation by pi about x composed with N(0, 0.3^2) axis-angle noise; joints
    BENT by 1.2 .. 2.8 rad about random axes, the others N(0, 0.3^2).  The 6-D columns leave the manifold without changing the rotation
    that Gram-Schmidt recovers: the second column is turned in the plane of the two to 15 .. 165 degrees from the first, then each
    column is scaled log-uniformly in [0.25, 4].  betas clip(N(0, 1.5^2), +-3); gt_j3d as synthetic_batch's: the joints of a pose 0.1
    rad of axis-angle noise per joint away, + N(0, 10^2) mm, pelvis-centred (targets=False: poses only, no gt_j3d)."""
    rng = np.random.RandomState(seed)
    rod = lambda aa: oracle.rodrigues(T(aa.reshape(-1, 3))).numpy().reshape(aa.shape[:-1] + (3, 3))
    aa = rng.normal(0.0, 0.3, size=(B, NJ, 3))
    ang = rng.uniform(1.2, 2.8, size=(B, len(BENT), 1))
    aa[:, BENT] = _unit(rng.standard_normal((B, len(BENT), 3))) * ang
    R = rod(aa)
    R[:, 0] = np.diag([1.0, -1.0, -1.0]) @ R[:, 0]
    phi = np.deg2rad(rng.uniform(15.0, 165.0, size=(B, NJ, 1)))
    scale = np.exp(rng.uniform(np.log(0.25), np.log(4.0), size=(B, NJ, 2)))
    a1 = R[..., 0] * scale[..., :1]
    a2 = (np.cos(phi) * R[..., 0] + np.sin(phi) * R[..., 1]) * scale[..., 1:]
    x6 = np.stack([a1, a2], -1).reshape(B, NJ, 6)                               # x[2 i + k] = column k, row i
    betas = np.clip(rng.normal(0.0, 1.5, size=(B, 10)), -3, 3)
    cam = np.tile(np.array([[0.0, 0.0, 2 * 5000 / (224 * 0.9)]]), (B, 1))
    out = dict(pose6d=x6.astype(np.float32), betas=betas.astype(np.float32), cam=cam.astype(np.float32), angles=np.linalg.norm(aa, axis=-1))
    if not targets:
        return out
    R_gt = R @ rod(rng.normal(0.0, 0.1, size=(B, NJ, 3)))
    smpl = oracle.OracleSMPL(model, dtype=torch.float64)
    Rg = T(R_gt)
    j = oracle.find_joints(smpl, T(betas), Rg[:, :1], Rg[:, 1:], T(np.maximum(np.asarray(J), 0)).double())
    gt = oracle.move_pelvis(j).numpy() * 1000.0 + rng.normal(0.0, 10.0, size=(B, 17, 3))
    gt = gt - gt[:, :1]
    out['gt_j3d'] = gt.astype(np.float32)
    return out


def column_geometry(x6d):
    """norms (B, 24, 2) of the two 6-D columns and the angle between them in degrees (B, 24)"""
    x = np.asarray(x6d, dtype=np.float64).reshape(-1, NJ, 3, 2)
    n = np.linalg.norm(x, axis=2)
    cosang = (x[..., 0] * x[..., 1]).sum(2) / (n[..., 0] * n[..., 1])
    return n, np.rad2deg(np.arccos(np.clip(cosang, -1, 1)))


def operator_inputs(sm, model, J, B: int, seed: int) -> torch.Tensor:
    """(B, 24, 6) float32 for the stand-alone discriminator operators: poses k % 3 == 0 from synthetic_batch, == 1 the 6-D values of
    far_batch (magnitudes up to 4), == 2 0.6 randn"""
    n = (B + 2) // 3
    rng = np.random.RandomState(seed)
    x = 0.6 * rng.standard_normal((B, NJ, 6))
    x[0::3] = sm.synthetic_batch(model, J, n, seed=seed)['pose6d'][:len(x[0::3])]
    x[1::3] = far_batch(model, J, n, seed=seed, targets=False)['pose6d'][:len(x[1::3])]
    return T(x.astype(np.float32))


# ---- the cases of the iteration tests ------------------------------------------------------------------------------------------------
BATCH_SEED = 3
_smpls, _built = {}, {}


def shipped_regressor(sm) -> np.ndarray:
    """the shipped H36M regressor (tests/golden/j_regressor_triplets.npz): 58 support vertices, the per-vertex iteration"""
    from conftest import load_golden
    t = load_golden('j_regressor_triplets.npz')
    return sm.j_regressor_from_triplets(t['rows'], t['cols'], t['vals'])


def smpls(model):
    """(fp32 oracle SMPL, fp64 oracle SMPL) of the surface body"""
    if 'surface' not in _smpls:
        _smpls['surface'] = (oracle.OracleSMPL(model), oracle.OracleSMPL(model, dtype=torch.float64))
    return _smpls['surface']


def build(sm, model, kind: str, B: int = B_CASE, support: str = 'h36m') -> dict:
    """support: 'h36m' (the shipped regressor) or a case of tests/support_cases.py ('n65': the tile lists).
    kind: 'formula' (oracle.formula_state_dict weights, synthetic_batch targets: what the suite had), 'dominant' / 'balanced'
    (strong pose weights, converged targets at 0.3 / 1.0 mm), 'shape' (strong shape weights, 0.3 mm), 'far' (far_batch, its own targets,
    no discriminator), 'far_disc' (far_batch with the strong pose weights).  Tensors: x6, betas, cam, gt_c (pelvis-centred mm), Jt;
    disc / shape_disc: the state dicts or None.  Built once per (kind, B, support), never modified."""
    key = (kind, B, support)
    if key in _built:
        return _built[key]
    if support == 'h36m':
        J = shipped_regressor(sm)
        c = dict(model=model, J=J, mask=None, support=np.nonzero((J > 0).any(0))[0])
    else:
        c = sc.build(model, support)
    J = sc.effective(c['J'], c['mask'])
    if kind in ('far', 'far_disc'):
        batch = far_batch(model, J, B, seed=BATCH_SEED)
    else:
        batch = dict(sm.synthetic_batch(model, J, B, seed=BATCH_SEED))
        if kind != 'formula':
            batch['gt_j3d'] = converged_targets(model, J, batch, NOISE_BALANCED if kind == 'balanced' else NOISE_DOMINANT)
    out = dict(name=f'{kind}/{support}', kind=kind, B=B, model=c['model'], body='surface', J=c['J'], mask=None, hint=None, support=c['support'],
               x6=T(batch['pose6d']), betas=T(batch['betas']), cam=T(batch['cam']), gt_c=oracle.move_pelvis(T(batch['gt_j3d'])),
               Jt=T(c['J']), mt=None, body_key=('surface', None),
               disc={'formula': oracle.formula_state_dict(oracle.DISC_PARAM_SHAPES, seed=0)}.get(kind,
                    strong_pose_disc() if kind in ('dominant', 'balanced', 'far_disc') else None),
               shape_disc=strong_shape_disc() if kind == 'shape' else None)
    if 'angles' in batch:
        out['angles'] = batch['angles']
    _built[key] = out
    return out


def oracle_parts(c, model, dtype, x6=None, betas=None, sub=slice(None), batch_norm=None, disc_x6=None):
    """the oracle's gradient (n, 154) = [pose | betas] at the case's state (or at x6 / betas) in `dtype`, split into the part without
    the discriminators and the discriminators' part; per-pose sums of (D - 1)^2.  disc_x6: the poses the discriminator part is taken
    at instead (the mutation check's stale hand-over)."""
    smpl = smpls(model)[0 if dtype == torch.float32 else 1]
    x = (c['x6'] if x6 is None else x6)[sub].to(dtype)
    b = (c['betas'] if betas is None else betas)[sub].to(dtype)
    gt, J = c['gt_c'][sub].to(dtype), c['Jt'].to(dtype)
    cast = lambda sd: None if sd is None else {k: v.to(dtype) for k, v in sd.items()}
    dsd, ssd = cast(c['disc']), cast(c['shape_disc'])
    _, gx, gb, _ = oracle.inner_grad(smpl, J, x, b, gt, batch_norm=batch_norm)
    base = torch.cat([gx.flatten(1), gb], 1)
    if dsd is None and ssd is None:
        return dict(base=base.double(), disc=torch.zeros_like(base).double(), pose_sq=None, shape_sq=None)
    if disc_x6 is None:
        _, gx, gb, _ = oracle.inner_grad(smpl, J, x, b, gt, dsd, ssd, batch_norm=batch_norm)
        full = torch.cat([gx.flatten(1), gb], 1)
        xd = x
    else:
        xd = disc_x6[sub].to(dtype)
        _, gxd, gbd, _ = oracle.inner_grad(smpl, J, xd, b, gt, dsd, ssd, batch_norm=batch_norm)
        _, gx0, gb0, _ = oracle.inner_grad(smpl, J, xd, b, gt, batch_norm=batch_norm)
        full = base + torch.cat([(gxd - gx0).flatten(1), gbd - gb0], 1)
    pose_sq = None if dsd is None else ((oracle.discriminator_forward(dsd, xd)[:, :, 0] - 1) ** 2).sum(1).double()
    shape_sq = None if ssd is None else ((oracle.shape_discriminator_forward(ssd, b)[:, 0] - 1) ** 2).double()
    return dict(base=base.double(), disc=(full - base).double(), pose_sq=pose_sq, shape_sq=shape_sq)


def rel_per_pose(a, b):
    a, b = a.double().flatten(1), b.double().flatten(1)
    return (a - b).norm(dim=1) / b.norm(dim=1)


def disc_share(p64, cols=slice(0, 144)):
    """|g_withD - g_withoutD| / |g_withD| per pose over the pose block (cols 0 .. 143) or the betas block (144 .. 153)"""
    full = p64['base'] + p64['disc']
    return p64['disc'][:, cols].norm(dim=1) / full[:, cols].norm(dim=1)


def oracle_step(c, model, n_iters: int = 1):
    """the fp32 oracle's state after n_iters iterations from the case's start (torch Adam, lr 1e-2): (x6, betas)"""
    o, p, b, _ = oracle.refine_poses(smpls(model)[0], c['Jt'], c['x6'][:, :1], c['x6'][:, 1:], c['betas'], c['gt_c'], n_iters,
                                     disc_sd=c['disc'], shape_disc_sd=c['shape_disc'])
    return torch.cat([o, p], 1), b
