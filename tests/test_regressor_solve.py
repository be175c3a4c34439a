"""The exact solve of the regressor fit without a GPU (regressor_solve.py): the loss and its gradient from the moments, the solver's
certificate, a planted regressor, the ring candidates, the flag rules and the schema of solve.json.  The moments are numpy float64
sums over the cases' rows (tests/jsolve_cases.py).

Bounds: the loss from the moments against the direct mean over the rows to rtol 1e-12; the gradient against central differences of
the loss (exact for a quadratic up to the rounding of the three evaluations: 1e-7 of the largest gradient entry); the solver to what
it promises, gap <= tol * L(x0) with tol = 1e-6 within jsolve_cases.MAX_ITER steps."""
import importlib
import json

import numpy as np
import pytest

import jsolve_cases as jc
from conftest import PKG_NAME

NAMES = sorted(jc.CASES)


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _moments(c):
    return jc.moments(jc.rows_of(c['points'], c['gt']))


_SOLVED = {}


def _solved(name, rings):
    """the solve of a case on its support (rings = 0) or its candidate lists (rings = 1), computed once"""
    if (name, rings) not in _SOLVED:
        c = jc.table(name)
        lists, x0 = (c['lists1'], c['x0_1']) if rings else (c['lists0'], c['x0'])
        M = _moments(c)
        _SOLVED[name, rings] = (M, lists, x0, _mod('regressor_solve').solve(M, c['n'], lists, x0, tol=jc.TOL, max_iter=jc.MAX_ITER))
    return _SOLVED[name, rings]


# ---- the loss and its gradient ----
@pytest.mark.parametrize('name', NAMES)
def test_loss_from_moments_is_the_direct_mean(name):
    rs = _mod('regressor_solve')
    c = jc.table(name)
    M = _moments(c)
    rng = np.random.RandomState(1)
    for lists, x in ((c['lists0'], c['x0']), (c['lists1'], c['x0_1']), (c['lists1'], jc.random_feasible(rng, c['lists1']))):
        got, want = rs.loss_from_moments(M, c['n'], lists, x)[0], jc.direct_loss(c['points'], c['gt'], lists, x)
        print(f'{name}: {got:.15e} against {want:.15e}, relative {abs(got - want) / want:.2e}')
        assert abs(got - want) <= 1e-12 * want


@pytest.mark.parametrize('name', NAMES)
def test_gradient_against_central_differences(name):
    rs = _mod('regressor_solve')
    c = jc.table(name)
    M, lists, x = _moments(c), c['lists1'], c['x0_1']
    _, grads = rs.loss_from_moments(M, c['n'], lists, x)
    assert [g.size for g in grads] == [l.size for l in lists]
    top = max(float(np.abs(g).max()) for g in grads if g.size)
    h, worst = 1e-3, 0.0
    for i in range(jc.NJ):
        for e in range(lists[i].size):
            xp, xm = [r.copy() for r in x], [r.copy() for r in x]
            xp[i][e] += h
            xm[i][e] -= h
            d = (rs.loss_from_moments(M, c['n'], lists, xp)[0] - rs.loss_from_moments(M, c['n'], lists, xm)[0]) / (2 * h)
            worst = max(worst, abs(d - grads[i][e]))
    print(f'{name}: gradient within {worst:.2e} of central differences (largest entry {top:.2e})')
    assert worst <= 1e-7 * top
    # a row without entries has no gradient and does not enter the loss
    for i in range(jc.NJ):
        if not lists[i].size:
            other = jc.rows_of(c['points'], c['gt']).copy()
            other[:, c['ns'] + i] += 100.0
            assert rs.loss_from_moments(jc.moments(other), c['n'], lists, x)[0] == pytest.approx(rs.loss_from_moments(M, c['n'], lists, x)[0], rel=1e-13)


# ---- the certificate ----
@pytest.mark.parametrize('rings', [0, 1])
@pytest.mark.parametrize('name', NAMES)
def test_certificate(name, rings):
    rs = _mod('regressor_solve')
    c = jc.table(name)
    M, lists, x0, r = _solved(name, rings)
    L0 = rs.loss_from_moments(M, c['n'], lists, x0)[0]
    L, grads = rs.loss_from_moments(M, c['n'], lists, r['x'])
    print(f'{name} rings {rings}: loss {L0:.6e} -> {L:.6e}, gap {r["gap"]:.3e} = {r["gap"] / L0:.2e} L(x0), {r["iterations"]} steps, '
          f'{sum(int((x > 0).sum()) for x in r["x"])} of {sum(l.size for l in lists)} entries positive')
    assert r['converged'] and r['gap'] <= jc.TOL * L0 and r['iterations'] <= jc.MAX_ITER
    assert r['loss'] == L and r['gap'] == rs.fw_gap(r['x'], grads) and r['gap'] >= 0.0      # the figures belong to the returned x
    assert abs(r['loss0'] - L0) <= 1e-12 * L0                                              # (x0 is normalised once more inside)
    for x, l in zip(r['x'], lists):
        assert x.size == l.size and (x >= 0).all()
        if l.size:
            assert abs(x.sum() - 1.0) <= 1e-12
    assert L <= L0
    rng = np.random.RandomState(2)
    floor = L - r['gap']
    for k in range(300):                                # Dirichlet points, and points near the solution, where a lower loss would lie
        y = jc.random_feasible(rng, lists) if k % 3 == 0 else jc.random_feasible(rng, lists, near=r['x'], scale=10.0 ** -rng.randint(1, 7))
        assert rs.loss_from_moments(M, c['n'], lists, y)[0] >= floor


def test_max_iter_ends_the_solve_unconverged():
    rs = _mod('regressor_solve')
    c = jc.table('body')
    r = rs.solve(_moments(c), c['n'], c['lists1'], c['x0_1'], tol=1e-12, max_iter=2)
    assert r['iterations'] == 2 and not r['converged'] and r['gap'] > 1e-12 * r['loss0'] and r['loss'] < r['loss0']
    with pytest.raises(ValueError):
        rs.solve(_moments(c), c['n'], c['lists1'], [-x for x in c['x0_1']])


def test_planted_regressor_is_recovered():
    """the ground truth comes from a simplex regressor inside the candidate lists, without noise (but rounded to float32): the optimum
    is (about) zero, so the certificate bounds the loss itself"""
    rs = _mod('regressor_solve')
    c = jc.table('planted')
    M, lists, x0, r = _solved('planted', 1)
    L0 = r['loss0']
    assert rs.loss_from_moments(M, c['n'], lists, c['x_true'])[0] <= 1e-3 * jc.TOL * L0      # the planted point is feasible and (nearly) exact
    rms = np.sqrt(jc.direct_loss(c['points'], c['gt'], lists, r['x']))
    print(f'planted: loss {L0:.6e} -> {r["loss"]:.3e} (tol L0 = {jc.TOL * L0:.3e}), rms joint residual {rms * 1000:.3e} mm')
    assert r['loss'] <= jc.TOL * L0
    assert rms <= np.sqrt(jc.TOL * L0)
    # on the support alone the planted regressor is out of reach: the solve there ends well above
    assert _solved('planted', 0)[3]['loss'] > 100 * jc.TOL * L0


# ---- rings ----
def test_ring_candidates_on_a_hand_made_mesh():
    rs = _mod('regressor_solve')
    J = np.zeros((3, 12), dtype=np.float32)
    J[0, 5] = 0.5
    J[1, [0, 3]] = 0.25, 0.75
    J[2, 11] = -1.0                                      # a negative entry is not in the support
    assert [v.tolist() for v in rs.ring_candidates(J, jc.GRID_FACES, 0)] == [[5], [0, 3], []]
    assert [v.tolist() for v in rs.ring_candidates(J, np.zeros((0, 3), dtype=np.int64), 0)] == [[5], [0, 3], []]
    # one ring: 5 touches 4, 6 (its row), 1, 9 (its column), 0 and 10 (the diagonals of its cells); 0 touches 1, 4, 5; 3 touches 2, 7
    assert [v.tolist() for v in rs.ring_candidates(J, jc.GRID_FACES, 1)] == [[0, 1, 4, 5, 6, 9, 10], [0, 1, 2, 3, 4, 5, 7], []]
    # two rings from 5: 1 adds 2, 4 adds 8, 6 adds 2, 7 and 11 -- everything but 3, which is three edges away (5 - 6 - 2 - 3);
    # two rings from 0 and 3: 4 adds 8 and 9, 5 adds 6, 9 and 10, 7 adds 6 and 11 -- everything
    assert [v.tolist() for v in rs.ring_candidates(J, jc.GRID_FACES, 2)] == [[0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11], list(range(12)), []]
    assert rs.ring_candidates(J, jc.GRID_FACES, 3)[0].tolist() == list(range(12))
    with pytest.raises(ValueError):
        rs.ring_candidates(J, jc.GRID_FACES, -1)
    with pytest.raises(ValueError):
        rs.ring_candidates(J, jc.GRID_FACES + 20, 1)
    P = rs.candidate_pattern(rs.ring_candidates(J, jc.GRID_FACES, 1), 12)
    assert P.shape == (3, 12) and P.sum(1).tolist() == [7, 7, 0] and P[0, 5] == 1


def test_ring_candidates_refuse_a_row_above_the_cap():
    """a strip of 400 vertices, every vertex in a triangle with its two successors: one ring reaches 2 vertices to either side"""
    rs = _mod('regressor_solve')
    faces = np.array([(a, a + 1, a + 2) for a in range(398)])
    J = np.zeros((17, 400), dtype=np.float32)
    J[3, 10:130:5] = 1.0                                 # 24 entries, 5 apart
    assert rs.ring_candidates(J, faces, 1)[3].tolist() == list(range(8, 128))       # 5 vertices each, side by side: 120, under the cap
    J[9, 200:328] = 1.0                                  # 128 entries: the cap itself
    assert rs.ring_candidates(J, faces, 0)[9].size == 128
    with pytest.raises(ValueError, match=r'row 9 has 132 candidate'):
        rs.ring_candidates(J, faces, 1)                  # 198 .. 329
    J[9] = 0
    J[3, 10:330:5] = 1.0                                 # 64 entries: two rings reach 4 to either side, the whole run 6 .. 329
    with pytest.raises(ValueError, match=r'row 3 has 324 candidate'):
        rs.ring_candidates(J, faces, 2)


@pytest.mark.parametrize('name', NAMES)
def test_a_larger_feasible_set_cannot_do_worse(name):
    r0, r1 = _solved(name, 0)[3], _solved(name, 1)[3]
    print(f'{name}: support {r0["loss"]:.6e}, candidates {r1["loss"]:.6e} (gap {r1["gap"]:.2e})')
    assert r1['loss'] <= r0['loss'] + r1['gap']
    assert r1['loss'] < r0['loss']                       # and on these cases, where the truth uses the candidates, it does better


# ---- flags and schema ----
def _ns(flags):
    return _mod('args').get_args(flags)


def test_flag_rules(tmp_path):
    rf = _mod('regressor_fit')
    vdir = tmp_path / 'meshes'
    vdir.mkdir()
    np.save(vdir / 'vertices.npy', np.zeros((1, 6890, 3), np.float32))
    ok = ['--fit_regressor', str(tmp_path / 'out'), '--fit_from', str(vdir)]
    table = ['--fit_regressor', 'out', '--fit_from', str(tmp_path / 'table'), '--data_root', str(tmp_path)]
    for flags in (ok + ['--fit_solve'], ok + ['--fit_solve', '--fit_rings', '0'], ok + ['--fit_solve', '--fit_rings', '1', '--synthetic'],
                  ok + ['--fit_solve', '--fit_rings', '2', '--smpl_dir', str(tmp_path)], table + ['--fit_solve', '--fit_rings', '1'],
                  ok + ['--fit_solve', '--fit_solve_tol', '1e-9', '--fit_solve_iters', '5']):
        rf.check_flags(_ns(flags))
    bad = [ok + ['--fit_rings', '1', '--synthetic'],                 # Adam cannot move a zero entry
           ok + ['--fit_solve', '--fit_rings', '1'],                # meshes without a body model: no faces
           ok + ['--fit_solve', '--fit_rings', '-1', '--synthetic'], ok + ['--fit_solve', '--fit_solve_tol', '0'],
           ok + ['--fit_solve', '--fit_solve_iters', '0'], ['--fit_solve'], ['--fit_rings', '1'],
           ok + ['--fit_solve', '--eval_report', 'd']]
    for flags in bad:
        with pytest.raises(ValueError):
            rf.check_flags(_ns(flags))
    ns = _ns(ok)
    assert ns.fit_solve is False and ns.fit_rings == 0 and ns.fit_solve_tol == 1e-6 and ns.fit_solve_iters >= 100


def test_solve_json_schema():
    rs, rf = _mod('regressor_solve'), _mod('regressor_fit')
    score = lambda a, b: {'mpjpe_mm': a, 'pampjpe_mm': b}
    before = {'train': score(60.0, 40.0), 'holdout': score(61.0, 41.0)}
    after = {'train': score(20.0, 15.0), 'holdout': score(22.0, 16.0)}
    ns = _ns(['--fit_regressor', 'out', '--fit_from', 'x', '--fit_solve', '--fit_rings', '1', '--synthetic'])
    res = {'x': None, 'loss': np.float64(2e-5), 'loss0': 1e-3, 'gap': np.float64(3e-10), 'iterations': np.int64(41), 'converged': np.bool_(True)}
    losses = {'train_before': 1e-3, 'train_after': 2e-5, 'holdout_before': 1.1e-3, 'holdout_after': 3e-5}
    doc = rs.build_doc('vertices', rf.flags_doc(ns), 86, 10, 1, [5] * 17, [30] * 17, [9] * 17, losses, res, 1e-6, before, after,
                       'out/retrained_J_Regressor.pt', 'init.npy')
    doc = json.loads(json.dumps(doc, sort_keys=True, default=str))
    assert sorted(doc) == sorted(rs.SOLVE_KEYS) and doc['layout_version'] == rs.LAYOUT_VERSION
    assert doc['rows'] == {'train': 86, 'holdout': 10} and doc['rings'] == 1
    assert sorted(doc['support']) == sorted(rs.SUPPORT_KEYS) and doc['support']['candidates'] == [30] * 17
    assert sorted(doc['loss']) == sorted(rs.LOSS_KEYS) and doc['loss']['train_after'] == 2e-5
    assert doc['gap'] == 3e-10 and doc['tol'] == 1e-6 and doc['iterations'] == 41 and doc['converged'] is True
    for side in (doc['initial'], doc['final']):
        assert sorted(side) == ['holdout', 'train'] and sorted(side['train']) == sorted(rf.SCORE_KEYS)
    for k in ('fit_regressor', 'fit_from', 'fit_solve', 'fit_rings', 'fit_solve_tol', 'fit_solve_iters', 'fit_holdout', 'j_regressor_init'):
        assert k in doc['flags'], k
    none = rs.build_doc('refined', {}, 5, 0, 0, [1] * 17, [1] * 17, [1] * 17, {'train_before': 1.0, 'train_after': 0.5}, res, 1e-6,
                        {'train': score(1.0, 1.0), 'holdout': None}, {'train': score(0.5, 0.5), 'holdout': None}, 'p', None)
    assert none['loss']['holdout_before'] is None and none['loss']['holdout_after'] is None and none['rows']['holdout'] == 0


def test_fit_json_keys_are_unchanged():
    """without --fit_solve nothing changes: the key tuple of fit.json is the one the epochs have always written"""
    rf = _mod('regressor_fit')
    assert rf.DOC_KEYS == ('layout_version', 'source', 'flags', 'rows', 'support', 'steps_per_epoch', 'epochs', 'initial', 'final', 'checkpoint',
                           'j_regressor_init')
    doc = rf.build_doc('vertices', {}, 5, 0, [1] * 17, [1] * 17, 1, {'train': {'mpjpe_mm': 1.0, 'pampjpe_mm': 1.0}, 'holdout': None}, [], 'p', None)
    assert sorted(doc) == sorted(rf.DOC_KEYS)


def test_the_header_declares_the_entry_points():
    import os
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, 'include', 'jrr.h')).read()
    for name in ('jrr_jfit_moments_bytes', 'jrr_jfit_moments', 'jrr_jfit_set_entries'):
        assert name + '(' in hdr and name in _mod('_lib').SIGNATURES
    assert 'jmom.hip' in _mod('build').SOURCES and 'jfitk.h' in _mod('build').HEADERS
