"""The evaluation report on the GPU (pytest -m gpu): jrr_evaluate_joints, jrr_regress_joints and jrr_eval_accumulate against the host
restatement (tests/eval_report_cases.py), the reference's stored values (tests/golden/g10_eval_joints.npz) and float64; `--eval_report`
and `--eval_vertices` through the drivers on synthetic batches; two gloo ranks on one GPU against one.

Bounds: every comparison with float64 is held to `3 x (the reference's float32 distance from float64 on THIS test's inputs) + 1e-7`
(eval_report_cases.bound); on float32 inputs oracle.reference_port equals the reference bit for bit (asserted by
tests/golden/make_golden_eval.py), so it stands for the reference where no value is stored.

Inputs: isotropic clouds (ec.pose_cases) and, since no skeleton looks like one, the families of ec.FAMILIES: body-shaped, thin, exactly
flat, nearly and exactly collinear, scaled, identical and constant poses, alone (B = 65), mixed in one wave (B = 130) and as stored
by the reference (tests/golden/g11_eval_degenerate.npz).

Shapes: B = 1, 63, 65, 130 around the 64-pose workgroup of k_evaluate_joints and its ragged last piece (63 * 17 and 65 * 17 floats
are no multiple of the 16-byte store); B = 3 and 70 meshes; the accumulator at B = 65 in one call and as 40 + 25.
"""
import importlib
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_report_cases as ec
import oracle
from conftest import PKG_NAME, ROOT, load_golden

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
F = np.float32


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


# ---- 1. jrr_evaluate_joints ----
def _reference_errors(pred, tgt, dtype):
    """the reference's per-joint errors (oracle.reference_port: the reference bit for bit on float32 inputs) in `dtype`"""
    p = T(pred).to(dtype)
    t = T(tgt).to(dtype) / 1000
    p = p - p[:, [0], :]
    t = t - t[:, [0], :]
    s1 = oracle.batch_compute_similarity_transform_torch(p, t)
    return torch.sqrt(((p - t) ** 2).sum(dim=-1)).numpy(), torch.sqrt(((s1 - t) ** 2).sum(dim=-1)).numpy()


@pytest.mark.parametrize('B,seed', [(1, 41), (63, 42), (65, ec.G10_POSE_SEED), (130, 12)])
def test_evaluate_joints_against_float64(B, seed):
    eng = _mod('engine')
    pred, tgt = ec.pose_cases(B, seed)
    e64, pa64 = _reference_errors(pred, tgt, torch.float64)
    e32, pa32 = _reference_errors(pred, tgt, torch.float32)
    d_plain, d_pa = np.abs(e32 - e64).max(), np.abs(pa32 - pa64).max()
    if seed == ec.G10_POSE_SEED:                       # the stored values of the reference itself
        g = load_golden('g10_eval_joints.npz')
        assert np.array_equal(pred, g['pred']) and np.array_equal(tgt, g['target_mm'])
        e32, pa32 = g['err_j'], g['err_pa_j']
        d_plain, d_pa = np.abs(e32 - e64).max(), np.abs(pa32 - pa64).max()
    err_j, err_pa_j = eng.evaluate_joints(T(pred).to(DEV), T(tgt).to(DEV))
    assert err_j.shape == (B, 17) and err_pa_j.shape == (B, 17)
    err_j, err_pa_j = err_j.cpu().numpy(), err_pa_j.cpu().numpy()
    g_plain, g_pa = np.abs(err_j - e64).max(), np.abs(err_pa_j - pa64).max()
    print(f'B {B}: plain {g_plain:.3e} (reference {d_plain:.3e}, bound {ec.bound(d_plain):.3e})  '
          f'PA {g_pa:.3e} (reference {d_pa:.3e}, bound {ec.bound(d_pa):.3e})  max error {e64.max():.2f} m')
    assert g_plain <= ec.bound(d_plain) and g_pa <= ec.bound(d_pa)
    assert np.abs(err_j - e32).max() <= ec.bound(d_plain) and np.abs(err_pa_j - pa32).max() <= ec.bound(d_pa)
    # the restatement under the same bound
    _, r_e, r_pa = ec.evaluate_joints(pred, tgt, torch.float32)
    assert np.abs(r_e - e64).max() <= ec.bound(d_plain) and np.abs(r_pa - pa64).max() <= ec.bound(d_pa)
    # the per-pose means jrr_evaluate returns, re-formed on the host in k_evaluate's own order
    m, m_pa = eng.evaluate(T(pred).to(DEV), T(tgt).to(DEV))
    h, h_pa = ec.pose_means(err_j, err_pa_j)
    same = np.array_equal(h, m.cpu().numpy()), np.array_equal(h_pa, m_pa.cpu().numpy())
    print(f'B {B}: means re-formed from the per-joint values bit-identical to jrr_evaluate: plain {same[0]}, PA {same[1]}')
    np.testing.assert_allclose(h, m.cpu().numpy(), rtol=1e-6, atol=0)
    assert np.abs(h_pa.astype(np.float64) - m_pa.cpu().numpy()).max() <= ec.bound(d_pa)


def test_evaluate_keeps_its_golden_values():
    """jrr_evaluate itself on G6 (its kernel's body moved into a shared header)"""
    eng = _mod('engine')
    g = load_golden('g6_evaluate.npz')
    err, err_pa = eng.evaluate(T(g['pred']).to(DEV), T(g['target_mm']).to(DEV))
    print('jrr_evaluate on g6:', [v.hex() for v in err.cpu().numpy().astype(np.float64)], [v.hex() for v in err_pa.cpu().numpy().astype(np.float64)])
    np.testing.assert_allclose(float(err.mean()) * 1000, float(g['mpjpe']), rtol=1e-5)
    np.testing.assert_allclose(float(err_pa.mean()) * 1000, float(g['pampjpe']), rtol=1e-4)


# ---- 1b. body-shaped, thin, flat, collinear, scaled, identical and constant poses (ec.FAMILIES) ----
def _distance(a, ref):
    """max |a - ref| over every value, float64; the NaN patterns must be equal, and an all-NaN pair is at distance 0"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(a), nan)
    return float(np.abs(a - ref)[~nan].max()) if not nan.all() else 0.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _device_errors(eng, pred, tgt):
    """(err_j, err_pa_j, mean, mean_pa) of jrr_evaluate_joints and jrr_evaluate as numpy arrays"""
    dp, dt = T(np.ascontiguousarray(pred)).to(DEV), T(np.ascontiguousarray(tgt)).to(DEV)
    return tuple(x.cpu().numpy() for x in eng.evaluate_joints(dp, dt) + eng.evaluate(dp, dt))


@pytest.fixture(scope='module')
def family_inputs():
    """per family its 65 poses (one full 64-pose workgroup and a ragged one), the reference in float64 and in float32 -- once"""
    out = {}
    for name in ec.FAMILIES:
        pred, tgt = ec.family_cases(name, 65)
        out[name] = (pred, tgt, _reference_errors(pred, tgt, torch.float64), _reference_errors(pred, tgt, torch.float32))
    return out


@pytest.mark.parametrize('name', list(ec.FAMILIES))
def test_evaluate_joints_on_every_family(family_inputs, name):
    """jrr_evaluate_joints and jrr_evaluate against float64 and against the float32 reference, every value of every pose, held to
    3 x (the reference's float32 distance from float64 on this family's inputs) + 1e-7.  What the K^T K eigen-decomposition this kernel had before gave on these inputs is in DESIGN.md section 3d."""
    eng = _mod('engine')
    pred, tgt, (e64, pa64), (e32, pa32) = family_inputs[name]
    assert np.isnan(pa64).all() == (name in ec.ALL_NAN_PA) and np.isnan(pa64).any() == (name in ec.ALL_NAN_PA)
    d_plain, d_pa = _distance(e32, e64), _distance(pa32, pa64)
    err_j, err_pa_j, m, m_pa = _device_errors(eng, pred, tgt)
    assert err_j.shape == (65, 17) and err_pa_j.shape == (65, 17) and m.shape == (65,) and m_pa.shape == (65,)
    with np.errstate(invalid='ignore'):
        finite = int(np.isfinite(err_pa_j).sum())
        worst = np.nanmax(np.where(np.isnan(pa64), 0, np.abs(err_pa_j.astype(np.float64) - pa64)))
    r_e, r_pa = ec.kernel_evaluate_joints(pred, tgt)
    print(f'{name}: PA worst {worst:.3e} (reference {d_pa:.3e}, bound {ec.bound(d_pa):.3e}), {finite} of {err_pa_j.size} finite; from the restatement: '
          f'plain {np.nanmax(np.abs(err_j - r_e)):.3e}, PA {np.nanmax(np.abs(err_pa_j - r_pa)) if name not in ec.ALL_NAN_PA else 0.0:.3e}')
    g_plain, g_pa = _distance(err_j, e64), _distance(err_pa_j, pa64)
    print(f'{name}: plain {g_plain:.3e} (reference {d_plain:.3e}, bound {ec.bound(d_plain):.3e})  PA {g_pa:.3e}  '
          f'from the float32 reference: plain {_distance(err_j, e32):.3e}, PA {_distance(err_pa_j, pa32):.3e}')
    assert g_plain <= ec.bound(d_plain) and g_pa <= ec.bound(d_pa)
    assert _distance(err_j, e32) <= ec.bound(d_plain) and _distance(err_pa_j, pa32) <= ec.bound(d_pa)
    if name == 'constant_target':
        assert not err_pa_j.any() and not m_pa.any()                                       # exactly 0, as the reference
    # jrr_evaluate: its per-pose means re-formed on the host from the per-joint values, in k_evaluate's own order
    h, h_pa = ec.pose_means(err_j, err_pa_j)
    np.testing.assert_allclose(h, m, rtol=1e-6, atol=0)
    g_mean = _distance(m_pa, h_pa)
    print(f'{name}: jrr_evaluate PA means from the re-formed ones {g_mean:.3e}, bit-identical {np.array_equal(h_pa, m_pa, equal_nan=True)}')
    assert g_mean <= ec.bound(d_pa)


def test_evaluate_joints_on_the_references_stored_degenerate_poses():
    """tests/golden/g11_eval_degenerate.npz: 8 poses each of six families with the reference's OWN float32 values; one launch of 48"""
    eng = _mod('engine')
    g = load_golden('g11_eval_degenerate.npz')
    e64, pa64 = _reference_errors(g['pred'], g['target_mm'], torch.float64)
    err_j, err_pa_j, m, m_pa = _device_errors(eng, g['pred'], g['target_mm'])
    h, h_pa = ec.pose_means(err_j, err_pa_j)
    n = ec.G11_POSES
    for k, name in enumerate(ec.G11_FAMILIES):
        sl = slice(k * n, (k + 1) * n)
        d_plain, d_pa = _distance(g['err_j'][sl], e64[sl]), _distance(g['err_pa_j'][sl], pa64[sl])
        got = _distance(err_j[sl], e64[sl]), _distance(err_pa_j[sl], pa64[sl]), _distance(err_j[sl], g['err_j'][sl]), _distance(err_pa_j[sl], g['err_pa_j'][sl])
        print(f'g11 {name}: from float64 plain {got[0]:.3e} PA {got[1]:.3e}; from the stored values plain {got[2]:.3e} PA {got[3]:.3e} '
              f'(reference {d_plain:.3e} / {d_pa:.3e}, bounds {ec.bound(d_plain):.3e} / {ec.bound(d_pa):.3e})')
        assert got[0] <= ec.bound(d_plain) and got[2] <= ec.bound(d_plain) and got[1] <= ec.bound(d_pa) and got[3] <= ec.bound(d_pa)
        assert _distance(m_pa[sl], h_pa[sl]) <= ec.bound(d_pa)
    np.testing.assert_allclose(h, m, rtol=1e-6, atol=0)


@pytest.fixture(scope='module')
def mixed_batch():
    """130 poses, pose b of family b mod 14: every wave holds every rank.  Each family's own batch of 10 and its references."""
    names = list(ec.FAMILIES)
    pred, tgt, fam, row = ec.mixed_cases(130)
    own = {k: ec.family_cases(k, 10) for k in names}
    return names, pred, tgt, fam, row, own


def test_mixed_ranks_in_one_wave_equal_each_family_alone(mixed_batch):
    """neither kernel has cross-lane arithmetic: a pose's values in the mixed batch have the BITS they have in a batch of their own
    family; and every value lies within its family's bound of float64"""
    eng = _mod('engine')
    names, pred, tgt, fam, row, own = mixed_batch
    mixed = _device_errors(eng, pred, tgt)
    e64, pa64 = _reference_errors(pred, tgt, torch.float64)
    e32, pa32 = _reference_errors(pred, tgt, torch.float32)
    for k, name in enumerate(names):
        alone = _device_errors(eng, *own[name])
        rows = np.flatnonzero(fam == k)
        assert np.array_equal(pred[rows], own[name][0][row[rows]])
        for a, b, what in zip(mixed, alone, ('err_j', 'err_pa_j', 'mean', 'mean_pa')):
            assert np.array_equal(_bits(a[rows]), _bits(b[row[rows]])), (name, what)
        d_plain, d_pa = _distance(e32[rows], e64[rows]), _distance(pa32[rows], pa64[rows])
        g_plain, g_pa = _distance(mixed[0][rows], e64[rows]), _distance(mixed[1][rows], pa64[rows])
        print(f'mixed {name}: plain {g_plain:.3e} ({ec.bound(d_plain):.3e})  PA {g_pa:.3e} ({ec.bound(d_pa):.3e})')
        assert g_plain <= ec.bound(d_plain) and g_pa <= ec.bound(d_pa), name
    nan_rows = np.flatnonzero(np.isnan(mixed[1]).any(1))
    assert nan_rows.tolist() == np.flatnonzero(fam == names.index('constant_pred')).tolist() and np.isfinite(mixed[0]).all()


def test_a_defective_pose_leaves_its_neighbours_bits_alone():
    """a constant pred gives NaN in its own 17 PA values and nowhere else; a pose with one NaN coordinate gives NaN in its own rows
    only; every other pose has the bits of the run without the defect"""
    eng = _mod('engine')
    pred, tgt = ec.family_cases('body', 130)
    clean = _device_errors(eng, pred, tgt)
    assert all(np.isfinite(x).all() for x in clean)
    constant = pred.copy()
    for b in (0, 5, 63, 64, 129):
        constant[b] = constant[b, 3]
    poisoned_pred, poisoned_tgt = pred.copy(), tgt.copy()
    poisoned_pred[7, 4, 1] = np.nan                     # one joint of a pred
    poisoned_tgt[70, 0, 2] = np.nan                     # the pelvis of a target: every distance of that pose
    for (p, t), bad in (((constant, tgt), [0, 5, 63, 64, 129]), ((poisoned_pred, poisoned_tgt), [7, 70])):
        got = _device_errors(eng, p, t)
        good = np.setdiff1d(np.arange(130), bad)
        for a, b, what in zip(got, clean, ('err_j', 'err_pa_j', 'mean', 'mean_pa')):
            assert np.array_equal(_bits(a[good]), _bits(b[good])), what
        assert np.isnan(got[1][bad]).all() and np.isnan(got[3][bad]).all()
    got = _device_errors(eng, constant, tgt)
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()                          # a constant pred: the plain errors are finite
    got = _device_errors(eng, poisoned_pred, poisoned_tgt)
    assert np.isnan(got[0][7]).tolist() == [i == 4 for i in range(17)] and np.isnan(got[0][70]).all() and np.isnan(got[2][[7, 70]]).all()


def test_accumulate_on_the_mixed_batch(mixed_batch):
    """one jrr_eval_accumulate call over the mixed batch: the restatement word for word, the constant-pred poses in BAD only"""
    eng = _mod('engine')
    names, pred, tgt, fam, row, own = mixed_batch
    err_j, err_pa_j = eng.evaluate_joints(T(pred).to(DEV), T(tgt).to(DEV))
    group = (np.arange(130) % 3).astype(np.int32)
    acc = _acc(3)
    eng.eval_accumulate(err_j, err_pa_j, T(group).to(DEV), 3, acc)
    want = ec.accumulate(err_j.cpu().numpy(), err_pa_j.cpu().numpy(), group, 3)
    np.testing.assert_array_equal(acc.cpu().numpy(), want)
    rows = want[:3 * ec.ROW].reshape(3, ec.ROW)
    bad = fam == names.index('constant_pred')
    assert bad.sum() == 9 and rows[:, ec.BAD].tolist() == [int((bad & (group == g)).sum()) for g in range(3)]
    assert rows[:, ec.COUNT].tolist() == [int((~bad & (group == g)).sum()) for g in range(3)] and want[-2] == 0 and want[-1] == 0
    assert rows[:, ec.HIST:ec.HIST + ec.BINS].sum() == 17 * 121 and rows[:, ec.HIST_PA:].sum() == 17 * 121
    # without the constant-pred poses the table is the same: they touched nothing but BAD
    keep = ~bad
    less = ec.accumulate(err_j.cpu().numpy()[keep], err_pa_j.cpu().numpy()[keep], group[keep], 3)
    less[:3 * ec.ROW].reshape(3, ec.ROW)[:, ec.BAD] = rows[:, ec.BAD]
    np.testing.assert_array_equal(less, want)


# ---- 2. jrr_regress_joints ----
@pytest.fixture(scope='module')
def meshes():
    """70 meshes whose first 3 are the fixture's"""
    return np.concatenate([ec.mesh_cases(ec.G10_MESHES, ec.G10_MESH_SEED), ec.mesh_cases(67, 23)])


def _regressor_cases():
    J = _mod('smpl_model').default_h36m_regressor()
    return {'joints_h36m': (J, np.ones_like(J)), 'joints_dense': (ec.dense_regressor(ec.G10_DENSE_SEED), None),
            'joints_dense_zero_row': (ec.dense_regressor(ec.G10_DENSE_SEED, ec.G10_ZERO_ROW), None)}


@pytest.mark.parametrize('key', ['joints_h36m', 'joints_dense', 'joints_dense_zero_row'])
def test_regress_joints_against_the_reference_and_float64(meshes, key):
    eng = _mod('engine')
    g = load_golden('g10_eval_joints.npz')
    J, mask = _regressor_cases()[key]
    table = eng.JointRegressorTable(T(J).to(DEV), None if mask is None else T(mask).to(DEV))
    out = {B: table.regress(T(meshes[:B]).to(DEV)).cpu().numpy() for B in (3, 70)}
    assert out[3].shape == (1, 3, 17, 3) and out[70].shape == (1, 70, 17, 3)
    assert np.array_equal(out[70][0, :3], out[3][0], equal_nan=True)                       # B = 70 against B = 3: equal bits
    for B in (3, 70):
        j64 = ec.regress(meshes[:B], J, mask, torch.float64)
        ref = g[key] if B == 3 else ec.regress(meshes[:B], J, mask, torch.float32)
        nan = np.isnan(j64)
        np.testing.assert_array_equal(np.isnan(ref), nan)
        np.testing.assert_array_equal(np.isnan(out[B][0]), nan)
        assert nan.any() == (key == 'joints_dense_zero_row') and (not nan.any() or nan[:, ec.G10_ZERO_ROW].all())
        d = np.abs(ref - j64)[~nan].max()
        got, got_ref = np.abs(out[B][0] - j64)[~nan].max(), np.abs(out[B][0] - ref)[~nan].max()
        print(f'{key} B {B}: {got:.3e} from float64, {got_ref:.3e} from the reference (reference {d:.3e}, bound {ec.bound(d):.3e})')
        assert got <= ec.bound(d) and got_ref <= ec.bound(d)


def test_regress_two_regressors_equal_two_calls(meshes):
    eng = _mod('engine')
    cases = _regressor_cases()
    v = T(meshes).to(DEV)
    for a, b, mask in (('joints_h36m', 'joints_dense', None), ('joints_dense_zero_row', 'joints_dense', None),
                       ('joints_h36m', 'joints_h36m', cases['joints_h36m'][1])):
        Ja, Jb = T(cases[a][0]).to(DEV), T(cases[b][0] * (F(1.5) if a == b else F(1))).to(DEV)
        m = None if mask is None else T(mask).to(DEV)
        both = eng.JointRegressorTable(torch.stack([Ja, Jb]), m).regress(v).cpu().numpy()
        one_a = eng.JointRegressorTable(Ja, m).regress(v).cpu().numpy()
        one_b = eng.JointRegressorTable(Jb, m).regress(v).cpu().numpy()
        assert both.shape == (2, 70, 17, 3)
        assert np.array_equal(both[0], one_a[0], equal_nan=True) and np.array_equal(both[1], one_b[0], equal_nan=True), (a, b)


def test_regress_on_the_engines_own_vertices(smpl_model_np):
    """vertices of find_joints_forward(return_verts=True): the joints equal the engine's own, H36M regressor and mask"""
    eng, sm = _mod('engine'), _mod('smpl_model')
    B = 70
    J = sm.default_h36m_regressor()
    batch = sm.synthetic_batch(smpl_model_np, J, B, seed=77)
    e = eng.RefineEngine(eng.DeviceModel(smpl_model_np, DEV), B, flags=eng.FLAG_KEEP_VERTS)
    mask = torch.ones(17, 6890, device=DEV)
    e.set_j_regressor(T(J).to(DEV), mask)
    joints, verts = e.find_joints_forward(T(batch['betas']).to(DEV), x6d=T(batch['pose6d']).to(DEV), return_verts=True)
    ours = eng.JointRegressorTable(T(J).to(DEV), mask).regress(verts).cpu().numpy()[0]
    v = verts.cpu().numpy()
    j64, j32 = ec.regress(v, J, np.ones_like(J), torch.float64), ec.regress(v, J, np.ones_like(J), torch.float32)
    d = np.abs(j32 - j64).max()
    got, got_eng = np.abs(ours - j64).max(), np.abs(ours - joints.cpu().numpy()).max()
    print(f'engine vertices: {got:.3e} from float64, {got_eng:.3e} from the engine\'s joints (reference {d:.3e}, bound {ec.bound(d):.3e})')
    assert got <= ec.bound(d) and got_eng <= ec.bound(d)


# ---- 3. jrr_eval_accumulate ----
def _acc(n_groups):
    return torch.zeros(n_groups * ec.ROW + ec.TRAILER, dtype=torch.int64, device=DEV)


def test_accumulate_equals_the_restatement_word_for_word():
    eng = _mod('engine')
    e0, e1, group = ec.accumulate_case()
    d0, d1, dg = T(e0).to(DEV), T(e1).to(DEV), T(group).to(DEV)
    acc = _acc(3)
    eng.eval_accumulate(d0, d1, dg, 3, acc)
    want = ec.accumulate(d0.cpu().numpy(), d1.cpu().numpy(), dg.cpu().numpy(), 3)          # the kernel's own read-back inputs
    np.testing.assert_array_equal(acc.cpu().numpy(), want)
    rows = want[:3 * ec.ROW].reshape(3, ec.ROW)
    assert not rows[1].any() and want[-2] == 2 and want[-1] == 0 and rows[:, ec.BAD].sum() == 3 and rows[:, ec.COUNT].sum() == 60
    two = _acc(3)                                       # 40 + 25 equal one call
    eng.eval_accumulate(d0[:40], d1[:40], dg[:40], 3, two)
    eng.eval_accumulate(d0[40:], d1[40:], dg[40:], 3, two)
    np.testing.assert_array_equal(two.cpu().numpy(), want)
    # an id >= n_groups sets trailer word 1 and leaves the rows untouched
    bad = _acc(3)
    g2 = dg[:4].clone()
    g2[:] = torch.tensor([3, 7, 1 << 30, 0], dtype=torch.int32)
    eng.eval_accumulate(d0[10:14], d1[10:14], g2, 3, bad)
    got = bad.cpu().numpy()
    np.testing.assert_array_equal(got, ec.accumulate(e0[10:14], e1[10:14], g2.cpu().numpy(), 3))
    assert got[-1] == 3 and got[0] == 1 and not got[ec.ROW:3 * ec.ROW].any()
    with pytest.raises(RuntimeError, match='3 poses carried a group id outside'):
        _mod('eval_report').derive(got, ['a', 'b', 'c'])


def test_eval_report_add_on_the_device():
    er = _mod('eval_report')
    pred, tgt = ec.pose_cases(130, 12)
    group = (np.arange(130) % 3).astype(np.int32)
    group[17] = -1
    rep = er.EvalReport(['a', 'b', 'c'], DEV)
    rep.add(T(pred[:64]).to(DEV), T(tgt[:64]).to(DEV), T(group[:64]).to(DEV))
    rep.add(T(pred[64:]).to(DEV), T(tgt[64:]).to(DEV), T(group[64:]).to(DEV))
    res = rep.finish()
    e64, pa64 = _reference_errors(pred, tgt, torch.float64)
    assert res['all']['n'] == 129 and res['ignored'] == 1 and res['all']['n_bad'] == 0
    keep = group == 1
    d = np.abs(_reference_errors(pred, tgt, torch.float32)[1] - pa64).max()
    np.testing.assert_allclose(res['groups']['b']['mpjpe_mm'], e64[keep].mean() * 1000, atol=1e-3)
    np.testing.assert_allclose(res['groups']['b']['pampjpe_per_joint_mm'], pa64[keep].mean(0) * 1000, atol=1000 * (ec.bound(d) + 2.0 ** -25))
    with pytest.raises(ValueError, match='int32 tensor on'):
        rep.add(T(pred[:4]).to(DEV), T(tgt[:4]).to(DEV), T(group[:4]))


# ---- 4. the drivers on synthetic batches (2 x 64) ----
SYN = ['--batch_size', '64', '--synthetic_batches', '2', '--synthetic', '--device', DEV, '--smpl_dir', '/nonexistent',
       '--j_regressor_init', '/nonexistent']


def _with_args(flags, fn):
    argsmod = _mod('args')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(flags)
    try:
        return fn()
    finally:
        argsmod._LazyArgs._ns = saved


@pytest.fixture(scope='module')
def driver_runs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp('eval_report'))
    sm = _mod('smpl_model')
    J = sm.default_h36m_regressor()
    J2 = (J * (1 + 0.5 * np.random.RandomState(5).rand(*J.shape))).astype(F)               # a regressor that differs from the initial one
    ck = os.path.join(tmp, 'retrained_J_Regressor.pt')
    _mod('checkpoint').save_j_regressor(T(J2), ck)
    flags = SYN + ['--eval_j_regressor', ck]
    evaluation = _mod('test')
    runs = {}
    for key, extra in (('plain', []), ('report', ['--eval_report', os.path.join(tmp, 'params')])):
        lines = []
        rep = _with_args(flags + extra, lambda: evaluation.test_pose_refiner_model(log=lines.append))
        runs[key] = (lines, rep)
    spec = importlib.util.spec_from_file_location('dump_eval_vertices', os.path.join(ROOT, 'tools', 'dump_eval_vertices.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    vdir = os.path.join(tmp, 'meshes')
    _with_args(flags, lambda: tool.main([vdir] + flags))
    lines = []
    _with_args(flags + ['--eval_vertices', vdir, '--eval_report', os.path.join(tmp, 'verts')],
               lambda: _mod('eval_report').evaluate_vertices(log=lines.append))
    runs['vertices_lines'] = lines
    return tmp, flags, runs


def test_eval_report_leaves_the_printed_lines_alone(driver_runs):
    tmp, flags, runs = driver_runs
    (plain_lines, plain), (lines, rep) = runs['plain'], runs['report']
    assert lines == plain_lines and len(lines) == 10 and 'eval_report' not in plain
    doc = _mod('eval_report').load(os.path.join(tmp, 'params'))
    assert sorted(os.listdir(os.path.join(tmp, 'params'))) == ['eval.json', 'eval.md']
    assert doc['source'] == 'parameters' and doc['groups'] == ['all'] and doc['flags']['batch_size'] == 64
    assert len(doc['j_regressor_retrained']['sha256_16']) == 16 and len(doc['j_regressor_initial']['sha256_16']) == 16
    for which in ('before', 'after'):
        r = doc['regressors'][which]['all']
        print(f"{which}: report {r['mpjpe_mm']!r} / {r['pampjpe_mm']!r}  printed {rep['mpjpe_' + which]!r} / {rep['pampjpe_' + which]!r}")
        assert r['n'] == 128 and r['n_bad'] == 0 and doc['regressors'][which]['ignored'] == 0
        assert abs(r['mpjpe_mm'] - rep['mpjpe_' + which]) <= 1e-3 and abs(r['pampjpe_mm'] - rep['pampjpe_' + which]) <= 1e-3
        assert sum(r['raw'][ec.HIST:ec.HIST + ec.BINS]) == 17 * 128
    b, a = doc['regressors']['before']['all'], doc['regressors']['after']['all']
    assert b['raw'] != a['raw'] and b['mpjpe_per_joint_mm'] != a['mpjpe_per_joint_mm']
    md = open(os.path.join(tmp, 'params', 'eval.md'), encoding='utf-8').read()
    assert f"| all | 128 | 0 | {b['mpjpe_mm']:.2f} → {a['mpjpe_mm']:.2f} |" in md and '| L_Wrist |' in md


def test_eval_vertices_agrees_with_the_parameter_path(driver_runs):
    tmp, flags, runs = driver_runs
    er = _mod('eval_report')
    v = np.load(os.path.join(tmp, 'meshes', 'vertices.npy'), mmap_mode='r')
    assert v.shape == (128, 6890, 3) and v.dtype == np.float32 and not os.path.exists(os.path.join(tmp, 'meshes', 'paths.txt'))
    params, verts = er.load(os.path.join(tmp, 'params')), er.load(os.path.join(tmp, 'verts'))
    assert verts['source'] == 'vertices' and len(runs['vertices_lines']) == 3
    for which in ('before', 'after'):
        p, q = params['regressors'][which]['all'], verts['regressors'][which]['all']
        print(f"{which}: parameters {p['mpjpe_mm']!r} / {p['pampjpe_mm']!r}  vertices {q['mpjpe_mm']!r} / {q['pampjpe_mm']!r}")
        assert q['n'] == 128 and q['n_bad'] == 0
        assert abs(p['mpjpe_mm'] - q['mpjpe_mm']) <= 1e-3 and abs(p['pampjpe_mm'] - q['pampjpe_mm']) <= 1e-3
        np.testing.assert_allclose(p['mpjpe_per_joint_mm'], q['mpjpe_per_joint_mm'], atol=1e-3)


def test_two_gloo_ranks_equal_one_rank(driver_runs):
    """main.py --eval_vertices under torchrun, two ranks over gloo sharing cuda:0 (64 meshes each, chunks of 48 + 16): every integer"""
    tmp, flags, runs = driver_runs
    er = _mod('eval_report')
    out = os.path.join(tmp, 'verts2')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1', '--master-port',
           '29583', os.path.join(ROOT, 'main.py')] + flags + ['--batch_size', '48', '--eval_vertices', os.path.join(tmp, 'meshes'),
                                                              '--eval_report', out, '--single_device', '--dist_backend', 'gloo']
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    one, two = er.load(os.path.join(tmp, 'verts')), er.load(out)
    assert sorted(os.listdir(out)) == ['eval.json', 'eval.md']
    for which in ('before', 'after'):
        assert two['regressors'][which]['all']['n'] == 128
        assert two['regressors'][which] == one['regressors'][which]
