"""The regressor fit without a GPU: the host restatement (tests/jfit_cases.py) against the oracle's normalisation and the golden J step,
the hold-out split, the minibatch schedule, the support lists, the flag rules, the schema of fit.json, the conditions the trajectory
case of the GPU tests was searched for, and the claim the feature rests on: under torch.optim.Adam an entry outside the initial
support lists keeps its bits."""
import importlib
import json

import numpy as np
import pytest
import torch

import jfit_cases as jc
import oracle
from conftest import load_golden, PKG_NAME

T = torch.from_numpy


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


# ---- the restatement ----
def test_restatement_normalises_as_the_oracle(j_h36m_np):
    J, mask, _, _ = jc.regressor_case(5)
    for Jx, mk in ((J, mask), (j_h36m_np, None)):
        want = oracle.normalize_j_regressor(T(Jx).double(), None if mk is None else T(mk).double()).numpy()
        got = jc.Restatement(Jx, mk, dtype=jc.F64).normalised()
        assert np.array_equal(got, want)
        assert np.allclose(got.sum(1), 1.0, atol=1e-12)


def test_restatement_reproduces_the_golden_j_step(j_h36m_np):
    """three Adam steps on the golden vertices (g2) change exactly the entries g8 lists, to its values"""
    g8, g2 = load_golden('g8_jstep.npz'), load_golden('g2_find_joints.npz')
    verts, gt_mm = g2['verts'].astype(np.float32), (g2['gt'].astype(np.float64) * 1000.0).astype(np.float32)
    r = jc.Restatement(j_h36m_np, np.ones_like(j_h36m_np), lr=1e-2, dtype=jc.F32)
    for _ in range(3):
        r.step(verts, gt_mm)
    J = r.raw()
    rows, cols = np.nonzero(J != j_h36m_np)
    assert rows.tolist() == g8['changed_rows'].tolist() and cols.tolist() == g8['changed_cols'].tolist()
    assert len(rows) == 62
    np.testing.assert_allclose(J[rows, cols], g8['new_vals'], rtol=0, atol=1e-6)


def test_restatement_gradient_is_the_oracles(smpl_model_np, j_h36m_np):
    """loss and gradient of one minibatch against oracle.j_regressor_loss_and_grad on the same meshes"""
    sm = _mod('smpl_model')
    batch = sm.synthetic_batch(smpl_model_np, j_h36m_np, 6, seed=31)
    x6d, betas = T(batch['pose6d']).double(), T(batch['betas']).double()
    gt_c = oracle.move_pelvis(T(batch['gt_j3d'])).double()
    smpl = oracle.OracleSMPL(smpl_model_np, dtype=torch.float64)
    loss, gJ, _ = oracle.j_regressor_loss_and_grad(smpl, T(j_h36m_np).double(), x6d[:, :1], x6d[:, 1:], betas, gt_c)
    R = oracle.rot6d_to_rotmat(x6d.reshape(-1, 6)).view(-1, 24, 3, 3)
    verts = smpl(global_orient=R[:, :1], body_pose=R[:, 1:], betas=betas, pose2rot=False).vertices
    r = jc.Restatement(j_h36m_np, None, dtype=jc.F64)
    r.J.data = T(j_h36m_np).double()
    pred = torch.matmul(jc.normalise(r.J, None)[None], verts)
    mine = torch.nn.MSELoss()(jc.move_pelvis(pred), gt_c / 1000)
    mine.backward()
    assert abs(mine.item() - float(loss)) <= 1e-12 * abs(float(loss))
    assert float((r.J.grad - gJ).abs().max()) <= 1e-10 * float(gJ.abs().max())


def test_entries_outside_the_lists_keep_their_bits():
    """the claim the feature rests on: 30 dense Adam steps of the restatement, float32 as the reference runs it -- an entry that is not
    positive in J_init * mask (zero, negative, or masked away) has g = m = v = 0 at every step and its bits never change"""
    c = jc.trajectory_case()
    J, mask, vtx = c['J'], c['mask'], c['vtx']
    listed = np.zeros(J.shape, dtype=bool)
    for i, v in enumerate(vtx):
        listed[i, v] = True
    assert np.array_equal(listed, (J * mask) > 0)
    assert (J[~listed] < 0).sum() == 34 and (mask[~listed] == 0).sum() == 2          # the case plants both kinds
    for name in ('f32', 'f64'):
        r = c[name]['final']
        m, v = r.moments()
        assert np.array_equal(r.raw()[~listed].astype(np.float32).view(np.uint32), J[~listed].view(np.uint32))
        assert not m[~listed].any() and not v[~listed].any()
        assert (r.raw()[listed] != J[listed]).all()


def test_trajectory_case_meets_the_conditions_it_was_searched_for():
    """asserted on the float64 run: an entry ends non-positive, every row keeps a positive one, no raw entry comes closer to zero than
    1e-5 at any step (a sign that the two precisions could disagree about would change relu'); the union is no multiple of 4"""
    c = jc.trajectory_case()
    vtx = c['vtx']
    listed = jc.to_lists(np.ones((jc.NJ, jc.V)), vtx) > 0
    raw = c['f64']['snaps'][-1]['raw']
    assert int(((raw <= 0) & listed).sum()) >= 1
    assert all(((raw[i] > 0) & listed[i]).any() for i in range(jc.NJ))
    assert c['f64']['closest'] >= 1e-5, c['f64']['closest']
    ns = len(np.unique(np.concatenate(vtx)))
    assert ns % 4 != 0 and [len(v) for v in vtx] == list(jc.COUNTS) and max(jc.COUNTS) == 128
    assert len(np.intersect1d(vtx[0], vtx[1])) >= 3
    d = max(jc.dist(a['raw'], b['raw']) for a, b in zip(c['f32']['snaps'], c['f64']['snaps']))
    print(f'NS {ns}, closest approach {c["f64"]["closest"]:.3e}, float32 against float64 after 30 steps {d:.3e}')
    assert c['f64']['losses'][-1] < c['f64']['losses'][0]


# ---- the host logic of regressor_fit ----
def _paths(n_seq, per_seq):
    return [f'/data/h36m/S9/Act {s // 4} 1/imageSequence/{s % 4 + 1}/img_{5 * (k + 1):06d}.jpg' for s in range(n_seq) for k in range(per_seq)]


def test_holdout_split_keeps_sequences_whole():
    rf, refined = _mod('regressor_fit'), _mod('refined')
    paths = _paths(20, 7)
    rng = np.random.RandomState(0)
    perm = rng.permutation(len(paths))
    paths = [paths[i] for i in perm] + ['/elsewhere/1.jpg', '/elsewhere/2.jpg']
    held = rf.holdout_split(len(paths), 0.1, paths)
    keys = [refined.sequence_key(p)[0] or f'#{i}' for i, p in enumerate(paths)]
    assert not ({k for k, h in zip(keys, held) if h} & {k for k, h in zip(keys, held) if not h})
    names = sorted({refined.sequence_key(p)[0] for p in paths[:-2]})
    assert {k for k, h in zip(keys, held) if h} == {names[9], names[19]}              # every 10th sequence of 22; the 22nd is not a 10th
    assert held.sum() == 14
    # F = 0.5: every second sequence, the keyless frames are sequences 21 and 22
    held = rf.holdout_split(len(paths), 0.5, paths)
    assert held.sum() == 10 * 7 + 1 and held[-1] and not held[-2]


def test_holdout_split_without_paths_and_without_a_fraction():
    rf = _mod('regressor_fit')
    assert not rf.holdout_split(50, 0.0, _paths(5, 10)).any()
    assert not rf.holdout_split(50, 0.0).any()
    held = rf.holdout_split(50, 0.1)
    assert held.tolist() == [False] * 45 + [True] * 5
    assert rf.holdout_split(96, 0.25).sum() == 24 and not rf.holdout_split(3, 0.1).any() and rf.holdout_split(0, 0.1).shape == (0,)
    with pytest.raises(ValueError):
        rf.holdout_split(10, 1.0)
    with pytest.raises(ValueError):
        rf.holdout_split(10, 0.1, ['a'] * 9)


def test_minibatch_schedule_has_a_short_last_batch():
    rf = _mod('regressor_fit')
    assert rf.schedule(150, 64) == [(0, 64), (64, 64), (128, 22)] == jc.schedule(150, 64)
    assert rf.schedule(128, 64) == [(0, 64), (64, 64)] and rf.schedule(3, 1) == [(0, 1), (1, 1), (2, 1)]
    assert rf.schedule(5, 4096) == [(0, 5)] and rf.schedule(0, 8) == []
    with pytest.raises(ValueError):
        rf.schedule(5, 0)


def test_support_lists_on_the_host():
    rf = _mod('regressor_fit')
    J, mask, cols400, vtx = jc.regressor_case(jc.TRAJECTORY_SEED)
    cols, counts, pos, got_vtx = rf.support_lists(J, mask)
    assert counts.tolist() == list(jc.COUNTS)
    assert np.array_equal(cols, np.unique(np.concatenate(vtx))) and np.all(np.diff(cols) > 0)
    for i in range(jc.NJ):
        assert np.array_equal(got_vtx[i], vtx[i]) and np.array_equal(cols[pos[i]], vtx[i])
    # a mask that removes a positive entry: it is in the list without the mask and not with it
    masked = np.flatnonzero((J[0] > 0) & (mask[0] == 0))
    assert masked.size == 1 and masked[0] not in vtx[0]
    assert masked[0] in rf.support_lists(J, None)[3][0] and rf.support_lists(J, None)[1][0] == jc.COUNTS[0] + 1
    # a shared vertex sits once in the union and at the same position in both rows' lists
    shared = np.intersect1d(vtx[0], vtx[1])
    assert shared.size >= 3 and len(cols) < sum(jc.COUNTS)
    for v in shared:
        assert pos[0][list(vtx[0]).index(v)] == pos[1][list(vtx[1]).index(v)] == list(cols).index(v)
    # 128 entries fit, 129 do not; no positive entry at all is refused as well
    J129 = J.copy()
    J129[1, np.setdiff1d(np.arange(jc.V), vtx[1])[0]] = 0.5
    with pytest.raises(ValueError, match='129'):
        rf.support_lists(J129, mask)
    with pytest.raises(ValueError, match='no positive'):
        rf.support_lists(-np.abs(J), mask)
    empty = J.copy()
    empty[3] = 0
    assert rf.support_lists(empty, mask)[1][3] == 0                                     # an empty row is accepted
    assert rf.support_counts(J, mask) == list(jc.COUNTS)


def _ns(flags):
    return _mod('args').get_args(flags)


def test_flag_conflicts_are_refused_before_anything_runs(tmp_path):
    rf = _mod('regressor_fit')
    vdir = tmp_path / 'meshes'
    vdir.mkdir()
    np.save(vdir / 'vertices.npy', np.zeros((1, 6890, 3), np.float32))
    ok = ['--fit_regressor', str(tmp_path / 'out'), '--fit_from', str(vdir)]
    rf.check_flags(_ns([]))
    rf.check_flags(_ns(ok))
    rf.check_flags(_ns(ok + ['--fit_holdout', '0', '--fit_epochs', '1', '--fit_shuffle']))
    rf.check_flags(_ns(['--fit_regressor', 'out', '--fit_from', str(tmp_path / 'table'), '--data_root', str(tmp_path)]))
    bad = [['--fit_from', str(vdir)], ['--fit_regressor', 'out'], ok + ['--eval_vertices', str(vdir)], ok + ['--smooth_refined', 'd'],
           ok + ['--fuse_refined', 'd'], ok + ['--save_refined', 'd'], ok + ['--init_refined', 'd'], ok + ['--eval_report', 'd'],
           ok + ['--regressor_report', 'd'], ok + ['--fit_epochs', '0'], ok + ['--fit_holdout', '1.0'], ok + ['--fit_holdout', '-0.1'],
           ok + ['--batch_size', '0'], ok + ['--j_reg_lr', '0'],
           ['--fit_regressor', 'out', '--fit_from', str(tmp_path / 'table')]]                  # a table without --data_root
    for flags in bad:
        with pytest.raises(ValueError):
            rf.check_flags(_ns(flags))
    ns = _ns(ok)
    assert ns.fit_epochs == 10 and ns.fit_holdout == 0.1 and ns.fit_shuffle is False


def test_fit_json_schema(tmp_path):
    rf = _mod('regressor_fit')
    score = lambda a, b: {'mpjpe_mm': a, 'pampjpe_mm': b}
    initial = {'train': score(60.0, 40.0), 'holdout': score(61.0, 41.0)}
    epochs = [dict(train=score(50.0 - k, 35.0), holdout=score(52.0, 36.0), epoch=k + 1, loss=1e-3 / (k + 1)) for k in range(3)]
    ns = _ns(['--fit_regressor', 'out', '--fit_from', 'x'])
    doc = rf.build_doc('vertices', rf.flags_doc(ns), 86, 10, [5] * 17, [4] * 17, 2, initial, epochs, 'out/retrained_J_Regressor.pt', 'init.npy')
    doc = json.loads(json.dumps(doc, sort_keys=True, default=str))
    assert sorted(doc) == sorted(rf.DOC_KEYS) and doc['layout_version'] == rf.LAYOUT_VERSION
    assert doc['rows'] == {'train': 86, 'holdout': 10} and doc['steps_per_epoch'] == 2
    assert doc['support'] == {'before': [5] * 17, 'after': [4] * 17}
    assert len(doc['epochs']) == 3 and doc['final'] == doc['epochs'][-1]
    for e in doc['epochs']:
        assert sorted(e) == sorted(rf.EPOCH_KEYS) and sorted(e['train']) == sorted(rf.SCORE_KEYS) == sorted(e['holdout'])
    assert sorted(doc['initial']) == ['holdout', 'train']
    for k in ('fit_regressor', 'fit_from', 'fit_epochs', 'fit_shuffle', 'fit_holdout', 'batch_size', 'j_reg_lr', 'seed', 'j_regressor_init'):
        assert k in doc['flags'], k
    none = rf.build_doc('refined', {}, 5, 0, [1] * 17, [1] * 17, 1, {'train': score(1.0, 1.0), 'holdout': None}, [], 'p', None)
    assert none['final'] == none['initial'] and none['rows']['holdout'] == 0
