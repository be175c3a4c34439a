"""jrr_evaluate_protocol on the GPU (pytest -m gpu): against the float64 restatement (tests/protocol_cases.py), the reference's stored
values (g13), jrr_evaluate_joints, its own table in exact integers, the bootstrap's units, and `--eval_protocol` / `--eval_gt_joints`
through the mesh evaluation.

Bounds: eval_report_cases.bound(d) = 3 d + 1e-7 with d the distance of the float32 restatement (the reference's arithmetic) from the
float64 one on the test's own inputs; no value is excluded.  Everything behind the fp32 per-joint errors is an integer: equality.

Shapes: 65 poses of mixed_cases -- every family of eval_report_cases.FAMILIES in one wave, a last workgroup of one pose --; batches
1, 63, 64, 65 and 130 for the ragged store (3 and 1 tail floats, a full wave, three workgroups); 70 meshes in chunks of 32 through
the driver."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_report_cases as ec
import protocol_cases as pc
from conftest import PKG_NAME, ROOT, load_golden

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
F, F64 = np.float32, np.float64
B0 = 65


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F)).view(np.int32)


def _run(pred, tgt, mask, root, unit=pc.TARGET_MM, group=None, n_groups=1, acc=None, rows=True):
    """(err_j, err_pa_j) numpy (None, None without rows) of one launch on host arrays"""
    g = None if group is None else T(np.asarray(group, dtype=np.int32)).to(DEV)
    e, pa = _mod('engine').evaluate_protocol(T(np.ascontiguousarray(pred)).to(DEV), T(np.ascontiguousarray(tgt)).to(DEV), mask, root, unit, g, n_groups, acc, rows)
    return (e.cpu().numpy(), pa.cpu().numpy()) if rows else (None, None)


@pytest.fixture(scope='module')
def mixed():
    """65 poses of every family, their metre targets (divided on the host in float32), and the restatement in both dtypes for every
    mask, root and unit (computed once, never changed)"""
    pred, tgt, fam, row = ec.mixed_cases(B0)
    tgt_m = (tgt / F(1000)).astype(F)
    ref = {}
    for mask_name, mask in pc.MASKS.items():
        for root_name, root in pc.ROOTS.items():
            for unit, t in ((pc.TARGET_MM, tgt), (pc.TARGET_M, tgt_m)):
                ref[mask_name, root_name, unit] = (pc.evaluate_protocol(pred, t, mask, root, unit, torch.float32), pc.evaluate_protocol(pred, t, mask, root, unit, torch.float64))
    return {'pred': pred, 'tgt': {pc.TARGET_MM: tgt, pc.TARGET_M: tgt_m}, 'fam': fam, 'ref': ref}


def _within(got, r32, r64, what):
    """got within bound(d) of the float64 restatement, d = the float32 restatement's own distance; NaN where, and only where, float64 has it"""
    d = pc.distance(r32, r64)
    assert np.array_equal(np.isnan(got), np.isnan(r64)), f'{what}: NaN pattern'
    err = pc.distance(got, r64)
    print(f'{what}: reference fp32 against float64 {d:.3e} m, bound {ec.bound(d):.3e} m, kernel against float64 {err:.3e} m')
    assert err <= ec.bound(d), what
    return d


# ---- 1. against float64 ----
@pytest.mark.parametrize('mask_name', list(pc.MASKS))
def test_every_mask_root_and_unit_against_float64(mixed, mask_name):
    mask = pc.MASKS[mask_name]
    out = [i for i in range(17) if not mask >> i & 1]
    for root_name, root in pc.ROOTS.items():
        for unit in (pc.TARGET_MM, pc.TARGET_M):
            (e32, pa32), (e64, pa64) = mixed['ref'][mask_name, root_name, unit]
            e, pa = _run(mixed['pred'], mixed['tgt'][unit], mask, root, unit)
            what = f'{mask_name} {root_name} {"mm" if unit == pc.TARGET_MM else "m"}'
            _within(e, e32, e64, what + ' plain')
            _within(pa, pa32, pa64, what + ' aligned')
            assert not _bits(e)[:, out].any() and not _bits(pa)[:, out].any(), what + ': excluded columns are +0.0f'
    if mask_name == 'one1':
        assert np.isnan(pa[:, 10]).all() and np.isfinite(e).all()
    else:
        assert np.isnan(pa).any(1).sum() == (mixed['fam'] == list(ec.FAMILIES).index('constant_pred')).sum()


# ---- 2. the reference's stored values ----
def test_g13_within_its_own_distance():
    g11, g13 = load_golden('g11_eval_degenerate.npz'), load_golden('g13_eval_protocol.npz')
    for mask_name in pc.G13_MASKS:
        for root_name, root in pc.ROOTS.items():
            mask = pc.MASKS[mask_name]
            e64, pa64 = pc.evaluate_protocol(g11['pred'], g11['target_mm'], mask, root, pc.TARGET_MM, torch.float64)
            e, pa = _run(g11['pred'], g11['target_mm'], mask, root)
            for key, got, r64 in (('err_j', e, e64), ('err_pa_j', pa, pa64)):
                stored = g13[pc.g13_key(mask_name, root_name, key)]
                d = _within(got, stored, r64, f'g13 {mask_name} {root_name} {key}')
                assert pc.distance(got, stored) <= ec.bound(d)


# ---- 3. the full mask against jrr_evaluate_joints ----
def test_full_mask_against_evaluate_joints(mixed):
    pred, tgt = mixed['pred'], mixed['tgt'][pc.TARGET_MM]
    (e32, pa32), (e64, pa64) = mixed['ref']['all17', 'joint0', pc.TARGET_MM]
    e, pa = _run(pred, tgt, pc.MASKS['all17'], pc.ROOT_JOINT0)
    old = [a.cpu().numpy() for a in _mod('engine').evaluate_joints(T(pred).to(DEV), T(tgt).to(DEV))]
    for name, got, was, r32, r64 in (('plain', e, old[0], e32, e64), ('aligned', pa, old[1], pa32, pa64)):
        d = pc.distance(r32, r64)
        assert np.array_equal(np.isnan(got), np.isnan(was))
        print(f'all17 joint0 mm {name}: bits equal to jrr_evaluate_joints: {np.array_equal(_bits(got), _bits(was))}; largest difference '
              f'{pc.distance(got, was.astype(F64)):.3e} m, bound {ec.bound(d):.3e} m')
        assert pc.distance(got, was.astype(F64)) <= ec.bound(d)


# ---- 4. a pose's result depends on the pose alone ----
@pytest.mark.parametrize('proto', ['lsp14_hips', 'h36m17'])
def test_batch_independence(proto):
    p = _mod('eval_protocol').PRESETS[proto]
    pred, tgt, _, _ = ec.mixed_cases(130)
    whole = [_bits(a) for a in _run(pred, tgt, p.joint_mask, p.root)]
    for B in (1, 63, 64, 65):
        part = [_bits(a) for a in _run(pred[:B], tgt[:B], p.joint_mask, p.root)]
        assert np.array_equal(part[0], whole[0][:B]) and np.array_equal(part[1], whole[1][:B]), B
    tail = [_bits(a) for a in _run(pred[67:], tgt[67:], p.joint_mask, p.root)]          # another place in the batch, another lane
    assert np.array_equal(tail[0], whole[0][67:]) and np.array_equal(tail[1], whole[1][67:])


# ---- 5. a joint outside the protocol is not read ----
def test_nan_in_an_excluded_joint_changes_no_bit(mixed):
    pred, tgt = mixed['pred'], mixed['tgt'][pc.TARGET_MM]
    ep = _mod('eval_protocol')
    for name, joints in (('lsp14', (7, 9)), ('lsp14_hips', (0,)), ('lsp14_hips', (0, 7, 9))):
        p = ep.PRESETS[name]
        clean = [_bits(a) for a in _run(pred, tgt, p.joint_mask, p.root)]
        dirty_pred, dirty_tgt = pred.copy(), tgt.copy()
        for j in joints:
            dirty_pred[::2, j, :] = np.nan
            dirty_tgt[1::3, j, 1] = np.nan
        dirty = [_bits(a) for a in _run(dirty_pred, dirty_tgt, p.joint_mask, p.root)]
        assert np.array_equal(clean[0], dirty[0]) and np.array_equal(clean[1], dirty[1]), (name, joints)
    # the root joint IS used, in M or not: joint 0 under lsp14
    p = ep.PRESETS['lsp14']
    dirty_pred = pred.copy()
    dirty_pred[3, 0, 0] = np.nan
    e, pa = _run(dirty_pred, tgt, p.joint_mask, p.root)
    assert np.isnan(e[3, list(p.joints)]).all() and not e[3, [0, 7, 9]].any() and np.isfinite(e[4]).all()


# ---- 6. the table ----
N_GROUPS = 3


def _accumulate_inputs():
    """(pred, target_mm, group) as eval_report_cases.accumulate_case arranges its values: group 1 empty, group -1 twice, a group >= n,
    a NaN pose, a value over the cap in an included joint (3) and one in an excluded joint (7), and a pose whose plain distances are
    exactly 0.05f, 0.15f and 0.1499999f under root joint 0 (target 0, pred joint 0 at 0: sqrtf(x * x) = x)"""
    pred, tgt = ec.pose_cases(B0, seed=17)
    pred, tgt = (pred * F(0.2)).astype(F), (tgt * F(0.2)).astype(F)
    group = np.where(np.random.RandomState(31).rand(B0) < 0.5, 0, 2).astype(np.int32)
    group[[5, 44]] = -1
    group[9] = N_GROUPS
    group[[1, 7, 50, 51]] = (0, 2, 0, 2)
    pred[7, 3, 1] = np.nan
    pred[50, 3, 0] = F(5e3)
    pred[51, 7, 0] = F(5e3)
    tgt[1], pred[1, 0] = 0, 0
    pred[1, 1], pred[1, 2], pred[1, 3] = (F(0.05), 0, 0), (0, F(0.15), 0), (0, 0, F(0.1499999))
    return pred, tgt, group


def _table():
    return torch.zeros(N_GROUPS * ec.ROW + ec.TRAILER, dtype=torch.int64, device=DEV)


@pytest.mark.parametrize('mask_name,root_name', [('lsp14', 'joint0'), ('lsp14', 'hips'), ('all17', 'joint0'), ('tri3', 'hips')])
def test_table_equals_the_integer_restatement_of_the_written_outputs(mask_name, root_name):
    mask, root = pc.MASKS[mask_name], pc.ROOTS[root_name]
    pred, tgt, group = _accumulate_inputs()
    acc = _table()
    e, pa = _run(pred, tgt, mask, root, group=group, n_groups=N_GROUPS, acc=acc)
    got = acc.cpu().numpy()
    assert np.array_equal(got, pc.accumulate(e, pa, group, N_GROUPS, mask))
    rows = got[:N_GROUPS * ec.ROW].reshape(N_GROUPS, ec.ROW)
    assert got[-2:].tolist() == [2, 1] and not rows[1].any()                  # ignored, bad group; the empty group
    included = 3 in pc.joints_of(mask), 7 in pc.joints_of(mask)
    assert int(rows[:, ec.BAD].sum()) == (1 + 1 if included[0] else 0) + (1 if included[1] else 0)
    assert int(rows[:, ec.COUNT].sum()) + int(rows[:, ec.BAD].sum()) == B0 - 3
    for j in range(17):
        if not mask >> j & 1:
            assert not rows[:, ec.SUM + j].any() and not rows[:, ec.SUM_PA + j].any(), j
    n = len(pc.joints_of(mask))
    assert np.array_equal(rows[:, ec.HIST:ec.HIST + ec.BINS].sum(1), n * rows[:, ec.COUNT]) and np.array_equal(rows[:, ec.HIST_PA:].sum(1), n * rows[:, ec.COUNT])
    if root == pc.ROOT_JOINT0 and mask >> 3 & 1:                             # the exact bin edges: 50 mm into bin 50, 150 mm and beyond into bin 150, 149.9999 into 149
        assert _bits(e[1, 1:4]).tolist() == _bits([F(0.05), F(0.15), F(0.1499999)]).tolist()
    # two calls on halves give the table of one call; the table alone, without the outputs, is the same table
    halves, alone = _table(), _table()
    _run(pred[:30], tgt[:30], mask, root, group=group[:30], n_groups=N_GROUPS, acc=halves)
    _run(pred[30:], tgt[30:], mask, root, group=group[30:], n_groups=N_GROUPS, acc=halves, rows=False)
    _run(pred, tgt, mask, root, group=group, n_groups=N_GROUPS, acc=alone, rows=False)
    assert np.array_equal(halves.cpu().numpy(), got) and np.array_equal(alone.cpu().numpy(), got)
    if mask_name == 'all17':                                                 # what jrr_eval_accumulate makes of the same two arrays
        old = _table()
        _mod('engine').eval_accumulate(T(e).to(DEV), T(pa).to(DEV), T(group).to(DEV), N_GROUPS, old)
        assert np.array_equal(old.cpu().numpy(), got)
    # group NULL: every pose in group 0
    single = torch.zeros(ec.ROW + ec.TRAILER, dtype=torch.int64, device=DEV)
    _run(pred, tgt, mask, root, n_groups=1, acc=single, rows=False)
    assert np.array_equal(single.cpu().numpy(), pc.accumulate(e, pa, None, 1, mask))


# ---- 7. the bootstrap ----
def test_unit_columns_sum_to_the_sum_words_of_the_protocol_table():
    eng, ep = _mod('engine'), _mod('eval_protocol')
    p = ep.PRESETS['lsp14']
    B, G = 200, 3
    pred, tgt = ec.pose_cases(B, seed=3)
    pred2 = (pred + np.random.RandomState(4).randn(*pred.shape).astype(F) * F(0.01)).astype(F)
    unit = (np.arange(B) // 4).astype(np.int32)                              # 50 units of 4 poses, unit u in group u % 3
    group = (unit % G).astype(np.int32)
    d_group, d_unit, gt = T(group).to(DEV), T(unit).to(DEV), T(tgt).to(DEV)
    errs, accs = [], []
    for q in (pred, pred2):
        acc = torch.zeros(G * ec.ROW + ec.TRAILER, dtype=torch.int64, device=DEV)
        e, e_pa = eng.evaluate_protocol(T(q).to(DEV), gt, p.joint_mask, p.root, ep.TARGET_MM, d_group, G, acc)
        errs += [e, e_pa]
        accs.append(acc.cpu().numpy()[:G * ec.ROW].reshape(G, ec.ROW))
    units = torch.zeros((50, 5), dtype=torch.int64, device=DEV)
    wins = torch.zeros(G * 8 + 3, dtype=torch.int64, device=DEV)
    eng.paired_units(*errs, d_group, d_unit, G, units, wins)
    units, wins = units.cpu().numpy(), wins.cpu().numpy()
    assert not accs[0][:, ec.BAD].any() and not accs[1][:, ec.BAD].any() and not wins[-3:].any()
    for g in range(G):
        col = units[np.arange(50) % G == g].sum(0)
        assert int(col[0]) == int(accs[0][g, ec.SUM:ec.SUM + 17].sum()) and int(col[1]) == int(accs[0][g, ec.SUM_PA:ec.SUM_PA + 17].sum())
        assert int(col[2]) == int(accs[1][g, ec.SUM:ec.SUM + 17].sum()) and int(col[3]) == int(accs[1][g, ec.SUM_PA:ec.SUM_PA + 17].sum())
        assert int(col[4]) == int(accs[0][g, ec.COUNT]) == int(wins[g * 8])


def test_paired_bootstrap_point_estimates_equal_the_reports_means():
    er, cr, ep = _mod('eval_report'), _mod('ci_report'), _mod('eval_protocol')
    p = ep.PRESETS['lsp14']
    B, names = 96, ['a', 'b']
    pred, tgt = ec.pose_cases(B, seed=5)
    pred2 = (pred + np.random.RandomState(6).randn(*pred.shape).astype(F) * F(0.01)).astype(F)
    group = (np.arange(B) % 2).astype(np.int32)
    d = [T(a).to(DEV) for a in (pred, pred2, tgt, group)]
    reports = {'before': er.EvalReport(names, DEV, p), 'after': er.EvalReport(names, DEV, p)}
    boot = cr.PairedBootstrap(names, *cr.unit_ids('frame', B), DEV, group, protocol=p)
    for lo, hi in ((0, 40), (40, B)):
        reports['before'].add(d[0][lo:hi], d[2][lo:hi], d[3][lo:hi])
        reports['after'].add(d[1][lo:hi], d[2][lo:hi], d[3][lo:hi])
        boot.add(d[0][lo:hi], d[1][lo:hi], (d[2][lo:hi], d[2][lo:hi]), d[3][lo:hi], np.arange(lo, hi))
    res = {k: r.finish(reduce=False) for k, r in reports.items()}
    ci = boot.finish(50, 1, 0.9, 'frame', reduce=False)
    for where, rb, ra, c in [('all', res['before']['all'], res['after']['all'], ci['all'])] + [(g, res['before']['groups'][g], res['after']['groups'][g], ci['groups'][g]) for g in names]:
        for key in ('mpjpe', 'pampjpe'):
            for which, r in (('before', rb), ('after', ra)):
                assert abs(c[key][which]['mean_mm'] - r[key + '_mm']) <= 1e-9 * r[key + '_mm'], (where, key, which)
        assert c['n_poses'] == rb['n'] and rb['mpjpe_per_joint_mm'][0] is None and rb['mpjpe_per_joint_mm'][1] is not None
    e, _ = pc.evaluate_protocol(pred, tgt, p.joint_mask, p.root, pc.TARGET_MM, torch.float64)
    assert abs(res['before']['all']['mpjpe_mm'] - e[:, list(p.joints)].mean() * 1000) <= 1e-3


# ---- 8. what is refused ----
def test_argument_errors_return_their_code_and_message():
    lib = _mod('_lib').load()
    P = ctypes.c_void_p
    pred, tgt = (torch.zeros(4, 17, 3, device=DEV) for _ in range(2))
    e, pa = (torch.full((4, 17), 7.0, device=DEV) for _ in range(2))
    acc = torch.zeros(ec.ROW + ec.TRAILER + 1, dtype=torch.int64, device=DEV)
    ok = dict(pred=pred.data_ptr(), tgt=tgt.data_ptr(), unit=0, mask=0x1FD7E, root=0, group=None, batch=4, n_groups=1, e=e.data_ptr(), pa=pa.data_ptr(),
              acc=acc.data_ptr())
    cases = [(dict(pred=None), b'pred and target'), (dict(tgt=None), b'pred and target'), (dict(e=None, pa=None, acc=None), b'no output'),
             (dict(mask=0), b'joint_mask'), (dict(mask=1 << 17), b'joint_mask'), (dict(mask=0x80000001), b'joint_mask'), (dict(root=2), b'root 2'),
             (dict(root=-1), b'root -1'), (dict(unit=2), b'target_unit 2'), (dict(batch=-1), b'batch -1'), (dict(n_groups=0), b'n_groups 0: 1 .. 1024'),
             (dict(n_groups=1025), b'n_groups 1025'), (dict(e=e.data_ptr() + 4), b'16-byte aligned'), (dict(pa=pa.data_ptr() + 8), b'16-byte aligned'),
             (dict(acc=acc.data_ptr() + 4), b'8-byte aligned')]
    for change, text in cases:
        a = dict(ok, **change)
        rc = lib.jrr_evaluate_protocol(P(a['pred']), P(a['tgt']), a['unit'], a['mask'], a['root'], P(a['group']), a['batch'], a['n_groups'], P(a['e']), P(a['pa']),
                                       P(a['acc']), None)
        assert rc == -1 and text in lib.jrr_last_error(), (change, rc, lib.jrr_last_error())
    a = dict(ok, n_groups=0, acc=None)                                       # n_groups is not looked at without a table; batch 0 launches nothing
    assert lib.jrr_evaluate_protocol(P(a['pred']), P(a['tgt']), 0, a['mask'], 0, None, 0, 0, P(a['e']), P(a['pa']), None, None) == 0
    torch.cuda.synchronize()
    assert bool((e == 7.0).all()) and bool((pa == 7.0).all()) and not bool(acc.any())          # nothing ran


# ---- 9. through the driver ----
def _main(flags, cwd):
    cmd = [sys.executable, os.path.join(ROOT, 'main.py')] + flags + ['--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent', '--synthetic', '--device', DEV]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


@pytest.fixture(scope='module')
def mesh_dirs(tmp_path_factory):
    """70 meshes of seeds in two actions of two cameras each, their ground-truth meshes, a perturbed regressor checkpoint; `regressed`
    holds no gt_j3d.npy, `file` links the same meshes and holds one"""
    tmp = tmp_path_factory.mktemp('protocol')
    n = 70
    model = _mod('smpl_model').synthetic_smpl(1234)
    J = _mod('smpl_model').default_h36m_regressor()
    J2 = (J * (1 + 0.5 * np.random.RandomState(5).rand(*J.shape))).astype(F)
    ck = str(tmp / 'retrained_J_Regressor.pt')
    _mod('checkpoint').save_j_regressor(T(J2), ck)
    rng = np.random.RandomState(12)
    t = (np.arange(n) // 2)[:, None, None]
    gt_verts = (model['v_template'][None] + 0.02 * np.sin(0.4 * t + rng.uniform(0, 6, size=(1, 6890, 3))) + rng.normal(0, 0.002, size=(n, 6890, 3))).astype(F)
    verts = (gt_verts * F(1.03) + rng.normal(0, 0.01, size=(n, 1, 3)) + 0.03 * np.sin(0.7 * t + rng.uniform(0, 6, size=(1, 6890, 3)))).astype(F)
    action = np.where(np.arange(n) < 40, 'Walking 1', 'Eating 2')
    paths = [f'/data/h36m/S9/{a}/imageSequence/{i % 2 + 1}/img_{5 * (i // 2 + 1):06d}.jpg' for i, a in enumerate(action)]
    a, b = str(tmp / 'regressed'), str(tmp / 'file')
    for d in (a, b):
        os.makedirs(d)
        with open(os.path.join(d, 'paths.txt'), 'w') as f:
            f.write('\n'.join(paths) + '\n')
    np.save(os.path.join(a, 'vertices.npy'), verts)
    np.save(os.path.join(a, 'gt_vertices.npy'), gt_verts)
    os.symlink(os.path.join(a, 'vertices.npy'), os.path.join(b, 'vertices.npy'))
    gt = (np.einsum('jv,nvc->njc', J.astype(F64), gt_verts.astype(F64)) * 1000 + rng.normal(0, 3, size=(n, 17, 3))).astype(F)
    np.save(os.path.join(b, 'gt_j3d.npy'), gt)
    return {'tmp': tmp, 'ck': ck, 'regressed': a, 'file': b, 'verts': verts, 'gt_verts': gt_verts, 'J': (J, J2), 'paths': paths}


def test_lsp14_hips_with_regressed_ground_truth_through_main(mesh_dirs):
    m = mesh_dirs
    cwd = str(m['tmp'] / 'run_a')
    os.makedirs(cwd)
    assert not os.path.exists(os.path.join(m['regressed'], 'gt_j3d.npy'))
    out = _main(['--batch_size', '32', '--eval_j_regressor', m['ck'], '--eval_vertices', m['regressed'], '--eval_report', 'rep', '--eval_protocol', 'lsp14_hips',
                 '--eval_gt_joints', 'regressed', '--eval_ci', '--eval_ci_reps', '200'], cwd)
    assert 'gt_j3d.npy is not read' in out
    er, cr = _mod('eval_report'), _mod('ci_report')
    rep = os.path.join(cwd, 'rep')
    assert sorted(os.listdir(rep)) == ['ci.json', 'ci.md', 'eval.json', 'eval.md']
    doc, ci = er.load(rep), cr.load(rep)
    entry = {'name': 'lsp14_hips', 'joints': [er.JOINT_NAMES[i] for i in pc.joints_of(pc.MASKS['lsp14'])], 'joint_mask': 0x1FD7E, 'root': 'hips',
             'gt_joints': 'regressed'}
    assert doc['protocol'] == entry and ci['protocol'] == entry and doc['flags']['eval_protocol'] == 'lsp14_hips' and doc['flags']['eval_gt_joints'] == 'regressed'
    assert doc['groups'] == ['Eating', 'Walking']
    group = np.array([0 if 'Eating' in p else 1 for p in m['paths']])
    mask = np.ones((17, 6890), dtype=F)
    for which, J in zip(('before', 'after'), m['J']):
        pj, gj = ec.regress(m['verts'], J, mask, torch.float64), ec.regress(m['gt_verts'], J, mask, torch.float64)
        e64, pa64 = pc.evaluate_protocol(pj, gj, pc.MASKS['lsp14'], pc.ROOT_HIPS, pc.TARGET_M, torch.float64)
        sel = pc.joints_of(pc.MASKS['lsp14'])
        for name, rows in (('Eating', group == 0), ('Walking', group == 1), ('all', group >= 0)):
            r = doc['regressors'][which]['all'] if name == 'all' else doc['regressors'][which]['groups'][name]
            want, want_pa = e64[rows][:, sel].mean() * 1000, pa64[rows][:, sel].mean() * 1000
            print(f'{which} {name}: n {r["n"]}  MPJPE {r["mpjpe_mm"]!r} (float64 {want!r})  PA-MPJPE {r["pampjpe_mm"]!r} (float64 {want_pa!r})')
            assert r['n'] == int(rows.sum()) and r['n_bad'] == 0                # counts are exact
            assert abs(r['mpjpe_mm'] - want) <= 1e-3 and abs(r['pampjpe_mm'] - want_pa) <= 1e-3
            assert [x is None for x in r['mpjpe_per_joint_mm']] == [i in (0, 7, 9) for i in range(17)]
            assert [x is None for x in r['pampjpe_per_joint_mm']] == [i in (0, 7, 9) for i in range(17)]
            c = ci['data']['all'] if name == 'all' else ci['data']['groups'][name]
            assert c['n_poses'] == r['n']
            for key in ('mpjpe', 'pampjpe'):                                 # the same integers behind both files
                assert abs(c[key][which]['mean_mm'] - r[key + '_mm']) <= 1e-9 * r[key + '_mm']
    assert doc['regressors']['before']['all']['mpjpe_mm'] != doc['regressors']['after']['all']['mpjpe_mm']
    md, cmd = (open(os.path.join(rep, f), encoding='utf-8').read() for f in ('eval.md', 'ci.md'))
    assert 'protocol lsp14_hips' in md.splitlines()[0] and 'protocol lsp14_hips' in cmd.splitlines()[0]
    assert 'Protocol `lsp14_hips`: 14 joints' in md and 'the midpoint of the hips' in cmd and 'regressed from the ground-truth meshes' in md
    assert ci['data']['reps'] == 200 and ci['data']['all']['n_units'] == 4


def test_parameter_path_keeps_its_printed_means_and_scores_the_protocol(tmp_path):
    """test_pose_refiner_model on one synthetic batch of 64 under lsp14: the ten printed lines are those of the default protocol (the
    reference's 17-joint evaluate), eval.json and ci.json carry the 14-joint numbers from the same integers"""
    argsmod, evaluation, er, cr = _mod('args'), _mod('test'), _mod('eval_report'), _mod('ci_report')
    J = _mod('smpl_model').default_h36m_regressor()
    ck = str(tmp_path / 'retrained_J_Regressor.pt')
    _mod('checkpoint').save_j_regressor(T((J * (1 + 0.5 * np.random.RandomState(5).rand(*J.shape))).astype(F)), ck)
    base = ['--batch_size', '64', '--synthetic_batches', '1', '--synthetic', '--device', DEV, '--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent',
            '--eval_j_regressor', ck, '--eval_ci', '--eval_ci_unit', 'frame', '--eval_ci_reps', '50']
    lines, docs = {}, {}
    for key, extra in (('h36m17', []), ('lsp14', ['--eval_protocol', 'lsp14'])):
        saved = argsmod._LazyArgs._ns
        argsmod._LazyArgs._ns = argsmod.get_args(base + extra + ['--eval_report', str(tmp_path / key)])
        try:
            lines[key] = []
            evaluation.test_pose_refiner_model(log=lines[key].append)
        finally:
            argsmod._LazyArgs._ns = saved
        docs[key] = (er.load(str(tmp_path / key)), cr.load(str(tmp_path / key)))
    assert lines['lsp14'][:10] == lines['h36m17'][:10] and len(lines['h36m17'][:10]) == 10
    (d17, c17), (d14, c14) = docs['h36m17'], docs['lsp14']
    assert 'protocol' not in d17 and 'protocol' not in c17 and d14['protocol']['name'] == c14['protocol']['name'] == 'lsp14' and d14['protocol']['gt_joints'] == 'file'
    for which in ('before', 'after'):
        r17, r14 = d17['regressors'][which]['all'], d14['regressors'][which]['all']
        assert r14['n'] == r17['n'] == 64 and r14['n_bad'] == 0
        assert [x is None for x in r14['mpjpe_per_joint_mm']] == [i in (0, 7, 9) for i in range(17)] and None not in r17['mpjpe_per_joint_mm']
        # the plain distance of a joint does not depend on the other joints: the 14 per-joint means are the 17-joint report's, to fp32 contraction
        for i in pc.joints_of(d14['protocol']['joint_mask']):
            assert abs(r14['mpjpe_per_joint_mm'][i] - r17['mpjpe_per_joint_mm'][i]) <= 1e-3, i
        assert abs(r14['mpjpe_mm'] - np.mean([r14['mpjpe_per_joint_mm'][i] for i in pc.joints_of(0x1FD7E)])) <= 1e-9
        for key in ('mpjpe', 'pampjpe'):
            assert abs(c14['data']['all'][key][which]['mean_mm'] - r14[key + '_mm']) <= 1e-9 * r14[key + '_mm']
        assert sum(r14['raw'][ec.HIST:ec.HIST + ec.BINS]) == 14 * 64 and sum(r17['raw'][ec.HIST:ec.HIST + ec.BINS]) == 17 * 64


def test_explicit_defaults_write_the_bytes_of_no_flags_at_all(mesh_dirs):
    m = mesh_dirs
    flags = ['--batch_size', '32', '--eval_j_regressor', m['ck'], '--eval_vertices', m['file'], '--eval_report', 'rep', '--eval_ci', '--eval_ci_reps', '50']
    outs = {}
    for key, extra in (('none', []), ('explicit', ['--eval_protocol', 'h36m17', '--eval_gt_joints', 'file'])):
        cwd = str(m['tmp'] / f'run_b_{key}')
        os.makedirs(cwd)
        outs[key] = (_main(flags + extra, cwd), os.path.join(cwd, 'rep'))
    assert outs['none'][0] == outs['explicit'][0]
    assert sorted(os.listdir(outs['none'][1])) == sorted(os.listdir(outs['explicit'][1])) == ['ci.json', 'ci.md', 'eval.json', 'eval.md']
    for name in os.listdir(outs['none'][1]):
        assert open(os.path.join(outs['none'][1], name), 'rb').read() == open(os.path.join(outs['explicit'][1], name), 'rb').read(), name
    doc = json.load(open(os.path.join(outs['none'][1], 'eval.json')))
    assert 'protocol' not in doc and 'eval_protocol' not in doc['flags'] and 'eval_gt_joints' not in doc['flags']
    assert None not in doc['regressors']['before']['all']['mpjpe_per_joint_mm'] and doc['regressors']['before']['all']['n'] == 70
