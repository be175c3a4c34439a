"""The inputs of tests/disc_cases.py without a GPU, on the float64 oracle: the conditions tests/test_gpu_adversarial_gradient.py relies
on, so that a later edit of a recipe cannot quietly make those tests blind -- full-rank weights, ReLU masks that differ from pose to
pose, outputs in both tails of the sigmoid, a discriminator share of the gradient that a comparison at max(3 e32, 2e-4) can see, a
yardstick e32 that leaves every bound meaningful, and a far batch that is far.  One mutation check on the oracle alone documents the
gap these inputs close: a discriminator gradient scaled by 1.002, or taken at the previous iteration's poses, passes the rule on the
formula-weight case the suite had and fails it on the new ones."""
import importlib

import numpy as np
import pytest
import torch

import disc_cases as dc
import oracle
from conftest import PKG_NAME

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope='module')
def sm():
    return importlib.import_module(PKG_NAME + '.smpl_model')


_memo = {}


def _measure(sm, model, kind, B=dc.B_CASE, support='h36m', sub=slice(None), batch_norm=None):
    """share of the discriminators in the pose block / the betas block, e32 over all 154 entries and over the betas block"""
    key = (kind, B, support)
    if key not in _memo:
        c = dc.build(sm, model, kind, B=B, support=support)
        p64 = dc.oracle_parts(c, model, F64, sub=sub, batch_norm=batch_norm)
        p32 = dc.oracle_parts(c, model, F32, sub=sub, batch_norm=batch_norm)
        g64, g32 = p64['base'] + p64['disc'], p32['base'] + p32['disc']
        _memo[key] = dict(c=c, p64=p64, p32=p32, g64=g64, g32=g32, share=dc.disc_share(p64), share_b=dc.disc_share(p64, slice(144, 154)),
                          e32=dc.rel_per_pose(g32, g64), e32_b=dc.rel_per_pose(g32[:, 144:], g64[:, 144:]))
    return _memo[key]


def test_formula_weights_are_what_the_issue_says(sm, smpl_model_np):
    """the starting point: rank 2, outputs near 0.5, masks that hardly depend on the pose, a share of 1e-5 .. 1e-4"""
    m = _measure(sm, smpl_model_np, 'formula')
    sd = m['c']['disc']
    assert int(torch.linalg.matrix_rank(sd['linear_operations.0.weight'].double(), rtol=1e-6)) == 2
    mixed, out = dc.pose_disc_activity(sd, m['c']['x6'])
    assert mixed['fc0'] < 0.05 and mixed['fc2'] < 0.01
    assert 0.45 < float(out.min()) and float(out.max()) < 0.55
    print(f'formula weights: share {m["share"].min():.2e} .. {m["share"].max():.2e}, median {m["share"].median():.2e}')
    assert float(m['share'].max()) < 2e-4 / 2                          # the whole term is below half the floor of the rule


@pytest.mark.parametrize('net', ['pose', 'shape'])
def test_strong_weights(net):
    sd = dc.strong_pose_disc() if net == 'pose' else dc.strong_shape_disc()
    shapes = oracle.DISC_PARAM_SHAPES if net == 'pose' else oracle.SHAPE_DISC_PARAM_SHAPES
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in shapes]
    assert all(v.dtype == torch.float32 and torch.isfinite(v).all() for v in sd.values())
    again = dc.strong_pose_disc() if net == 'pose' else dc.strong_shape_disc()
    assert all(torch.equal(sd[k], again[k]) for k in sd)                                      # seeded
    for k, w in dc.weight_matrices(sd).items():
        assert int(torch.linalg.matrix_rank(w)) == min(w.shape), k


def test_pose_masks_and_outputs(sm, smpl_model_np):
    c = dc.build(sm, smpl_model_np, 'dominant')
    mixed, out = dc.pose_disc_activity(c['disc'], c['x6'])
    print('strong pose weights: mixed units', {k: round(v, 3) for k, v in mixed.items()},
          f'outputs {out.min():.3f} .. {out.max():.3f}, 5 % / 95 % quantiles {out.flatten().quantile(0.05):.3f} / {out.flatten().quantile(0.95):.3f}')
    assert set(mixed) == {'conv0', 'conv2', 'fc0', 'fc2'} and min(mixed.values()) >= 0.3, mixed
    assert float(out.min()) < 0.1 and float(out.max()) > 0.9
    assert float(out.flatten().quantile(0.05)) < 0.15 and float(out.flatten().quantile(0.95)) > 0.85      # both tails are populated


def test_shape_masks_and_outputs(sm, smpl_model_np):
    c = dc.build(sm, smpl_model_np, 'shape', B=37)
    mixed, out = dc.shape_disc_activity(c['shape_disc'], c['betas'])
    print('strong shape weights: mixed units', mixed, f'outputs {out.min():.3f} .. {out.max():.3f}')
    assert min(mixed.values()) >= 0.3, mixed
    assert float(out.min()) < 0.1 and float(out.max()) > 0.9


CASES = [('dominant', 64, 'h36m'), ('balanced', 64, 'h36m'), ('dominant', 64, 'n65'), ('balanced', 64, 'n65'), ('dominant', 544, 'h36m'),
         ('balanced', 544, 'h36m'), ('shape', 37, 'h36m'), ('far', 33, 'h36m'), ('far_disc', 33, 'h36m')]


@pytest.mark.parametrize('kind,B,support', CASES)
def test_share_and_yardstick(sm, smpl_model_np, kind, B, support):
    """the discriminator share per pose and the fp32 oracle's own error, on the poses the GPU test compares (B = 544: 17 strided
    poses with batch_norm = 544)"""
    sub, bn = (slice(3, 544, 32), 544) if B == 544 else (slice(None), None)
    m = _measure(sm, smpl_model_np, kind, B, support, sub, bn)
    print(f'{kind} B = {B} {support}: pose share {m["share"].min():.3f} .. {m["share"].max():.3f}, betas share {m["share_b"].min():.3f} .. '
          f'{m["share_b"].max():.3f}, e32 <= {m["e32"].max():.2e}, betas alone <= {m["e32_b"].max():.2e}, |g64| {m["g64"].norm(dim=1).min():.2e} .. '
          f'{m["g64"].norm(dim=1).max():.2e}')
    assert 3 * float(m['e32'].max()) <= 2e-3 and 3 * float(m['e32_b'].max()) <= 2e-3            # no bound of the GPU tests is vacuous
    if kind == 'dominant':
        assert float(m['share'].min()) >= 0.3
    if kind == 'balanced':
        assert 0.1 <= float(m['share'].min()) and float(m['share'].median()) <= 0.9                # both terms matter
        if (B, support) == (64, 'h36m'):
            assert float(m['share'].max()) <= 0.9              # ... for every pose of the main case (n65: a few poses reach 0.96)
    if kind == 'shape':
        assert float(m['share_b'].min()) >= 0.3
    if kind == 'far':
        assert 3 * float(m['e32'].max()) < dc.G_FLOOR                                            # the floor decides


def test_far_batch_is_far(sm, smpl_model_np):
    c = dc.build(sm, smpl_model_np, 'far', B=33)
    x = c['x6'].numpy()
    norms, angles = dc.column_geometry(x)
    assert (c['angles'][:, list(dc.BENT)] >= 1.2).all() and c['angles'].max() > 2.5
    assert norms.min() < 0.5 and norms.max() > 2.0 and 0.25 <= norms.min() and norms.max() <= 4.0
    assert angles.min() < 30.0 and angles.max() > 150.0
    assert np.abs(x).max() > 2.5                                                                  # what the discriminator reads
    # the root is upside down, and Gram-Schmidt still recovers rotations
    R = oracle.rot6d_to_rotmat(c['x6'].double().reshape(-1, 6)).view(-1, 24, 3, 3)
    assert (R[:, 0, 1, 1] < 0).all() and (R[:, 0, 2, 2] < 0).all()
    assert (R.transpose(-1, -2) @ R - torch.eye(3, dtype=F64)).abs().max() < 1e-6
    theta = torch.acos(((R.diagonal(dim1=-2, dim2=-1).sum(-1) - 1) / 2).clamp(-1, 1))
    assert float(theta[:, list(dc.BENT)].min()) > 1.19 and float(theta.max()) > 2.5
    assert np.abs(c['betas'].numpy()).max() > 2.0 and np.abs(c['betas'].numpy()).max() <= 3.0
    assert (c['gt_c'][:, 0] == 0).all()
    again = dc.far_batch(smpl_model_np, dc.shipped_regressor(sm), 33, seed=dc.BATCH_SEED)
    assert np.array_equal(again['pose6d'], x)                                                     # seeded


def test_far_batch_three_oracle_iterations(sm, smpl_model_np):
    """three oracle iterations from the far batch in fp32 against fp64: 1.0e-6 at B = 16.  At the GPU test's B = 33 two of the 4752
    pose entries have |g64| of 2e-8 and 3e-8, next to Adam's eps of 1e-8, where the step g / (|g| + eps) turns rounding into 4.9e-4 and
    1.2e-5 of difference between the two oracles; every other entry stays below 1e-5 (mean 1.4e-7)."""
    smpl32, smpl64 = dc.smpls(smpl_model_np)
    for B, bound, n_loose in ((16, 1e-5, 0), (33, 6e-4, 2)):
        c = dc.build(sm, smpl_model_np, 'far', B=B)
        o, p, b, _ = oracle.refine_poses(smpl32, c['Jt'], c['x6'][:, :1], c['x6'][:, 1:], c['betas'], c['gt_c'], 3)
        o64, p64, b64, _ = oracle.refine_poses(smpl64, c['Jt'].double(), c['x6'][:, :1].double(), c['x6'][:, 1:].double(), c['betas'].double(),
                                               c['gt_c'].double(), 3)
        d = (torch.cat([o, p], 1) - torch.cat([o64, p64], 1)).abs()
        print(f'far batch B = {B}: three oracle iterations fp32 against fp64: max {d.max():.2e} mean {d.mean():.2e}, '
              f'{int((d > 1e-5).sum())} entries above 1e-5, betas {(b - b64).abs().max():.2e}')
        assert torch.isfinite(o).all() and torch.isfinite(p).all()
        assert float(d.max()) < bound and int((d > 1e-5).sum()) <= n_loose and float(d.mean()) < 1e-6
        assert float((b - b64).abs().max()) < 1e-5


def test_converged_targets(sm, smpl_model_np):
    J = dc.shipped_regressor(sm)
    batch = sm.synthetic_batch(smpl_model_np, J, 8, seed=1)
    own = dc._joints64_mm(smpl_model_np, J, batch['pose6d'], batch['betas'])
    for noise in (0.0, 0.3, 1.0):
        gt = dc.converged_targets(smpl_model_np, J, batch, noise)
        assert gt.dtype == np.float32 and gt.shape == (8, 17, 3) and (gt[:, 0] == 0).all()
        d = gt[:, 1:] - own[:, 1:]
        if noise == 0.0:
            assert np.abs(d).max() < 1e-3                                                         # fp32 rounding of some hundred mm
        else:
            assert 0.8 * noise < d.std() < 1.7 * noise                                            # (re-centring adds the pelvis' noise)


def _mutants(sm, model, kind, support='h36m'):
    """err / bound per pose of the two mutants of the fp32 oracle's gradient: the discriminator part scaled by 1.002 (at the start
    state), and taken at the previous iteration's poses (at the state after one oracle iteration)"""
    m = _measure(sm, model, kind, support=support)
    c, g64 = m['c'], m['g64']
    bound = torch.clamp(3 * m['e32'], min=dc.G_FLOOR)
    scaled = dc.rel_per_pose(m['p32']['base'] + 1.002 * m['p32']['disc'], g64) / bound
    x1, b1 = dc.oracle_step(c, model, 1)
    q64 = dc.oracle_parts(c, model, F64, x6=x1, betas=b1)
    q32 = dc.oracle_parts(c, model, F32, x6=x1, betas=b1)
    qs = dc.oracle_parts(c, model, F32, x6=x1, betas=b1, disc_x6=c['x6'])
    h64 = q64['base'] + q64['disc']
    bound1 = torch.clamp(3 * dc.rel_per_pose(q32['base'] + q32['disc'], h64), min=dc.G_FLOOR)
    assert (dc.rel_per_pose(q32['base'] + q32['disc'], h64) <= bound1).all()
    stale = dc.rel_per_pose(qs['base'] + qs['disc'], h64) / bound1
    return scaled, stale


def test_mutants_pass_on_the_old_case_and_fail_on_the_new_ones(sm, smpl_model_np):
    """Measured: formula weights -- scaled mutant at most 0.012 of the bound, stale mutant at most 0.51; dominant -- 4.2 .. 9.7 and
    2.8 .. 65 times the bound; balanced -- 2.2 .. 8.1 and 2.4 .. 63.  (On the dense 33-vertex regressor of
    test_gpu_support_shapes.py::test_one_iteration_with_pose_disc the joint gradient is some ten times smaller and the formula
    weights' stale mutant reaches 3.8 times the bound for a few poses; that test runs one iteration, where nothing can be stale.)"""
    scaled, stale = _mutants(sm, smpl_model_np, 'formula')
    print(f'formula: scaled <= {scaled.max():.3f}, stale <= {stale.max():.3f} of the bound')
    assert (scaled <= 1).all() and (stale <= 1).all()                  # every pose passes: the suite could not see either
    for kind in ('dominant', 'balanced'):
        scaled, stale = _mutants(sm, smpl_model_np, kind)
        print(f'{kind}: scaled {scaled.min():.2f} .. {scaled.max():.2f}, stale {stale.min():.2f} .. {stale.max():.2f} times the bound')
        assert (scaled > 1).all() and (stale > 1).all()                # every pose fails
