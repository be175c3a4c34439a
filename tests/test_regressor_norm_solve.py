"""The MPJPE solve of the regressor fit without a GPU (regressor_solve.py: norm_blocks_reference, norm_objective, norm_gradient,
solve_quadratic_blocks, solve_norm): the passes are the numpy restatement of jrr_jfit_norm_moments, through the same callback the
device pass goes through.  Inputs: tests/jnorm_cases.py.

Bounds.  The gradient against central differences of L_delta at step h = 1e-6 (delta = 1e-4 m keeps the third derivative, of the order
of |p|^3 / delta^2, small against it): 1e-6 of the largest gradient entry plus the rounding of the difference quotient, 1e-16 / h.  The
majoriser: Q(y) >= L_delta(y) - 1e-15 at random pairs, with equality at y = x.  The solver to what it promises: L_delta never rises
(to one rounding of a 10 200-term sum, 1e-13 relative), gap <= tol * L_delta(x0), and L(x) <= L(x') + gap + delta for every feasible x'.
"""
import importlib
import json
import os

import numpy as np
import pytest

import jnorm_cases as nc
import jsolve_cases as jc
from conftest import PKG_NAME, ROOT

DELTA = 1e-5            # m: the command's default, 0.01 mm
TOL = 1e-6


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _pass_fn(c):
    rs = _mod('regressor_solve')
    return lambda x, mode, delta: rs.norm_blocks_reference(c['rows'], c['lists'], x, mode, delta)


_SOLVED = {}


def _solved(name, tol=TOL):
    if (name, tol) not in _SOLVED:
        c = nc.table(name)
        _SOLVED[name, tol] = _mod('regressor_solve').solve_norm(_pass_fn(c), c['n'], c['lists'], c['x0'], DELTA, tol=tol, max_iter=400)
    return _SOLVED[name, tol]


def _worst(x, y):
    return max(float(np.abs(a - b).max()) for a, b in zip(x, y) if a.size)


# ---- the pass ----
@pytest.mark.parametrize('name', ['shipped', 'empty_row', 'empty_pelvis', 'wide'])
@pytest.mark.parametrize('mode', [nc.UNIT, nc.INV])
def test_the_reference_pass_is_the_definition(name, mode):
    rs = _mod('regressor_solve')
    c = nc.table(name)
    got = rs.norm_blocks_reference(c['rows'], c['lists'], c['x0'], mode, DELTA)
    want = nc.blocks(c['rows'], c['lists'], c['x0'], mode, DELTA)
    counts = [l.size for l in c['lists']]
    offs = rs.norm_block_offsets(counts)
    assert len(got) == 17 and got[0] is None and len(offs) == 17
    flat = np.zeros(offs[-1])
    for i in range(1, 17):
        K = counts[i] + counts[0] if counts[i] else 0
        assert got[i]['A'].shape == (K, K) and got[i]['b'].shape == (K,) and got[i]['cnt'] == counts[i]
        assert got[i]['n'] == (c['n'] if K else 0)
        for k in ('A', 'b', 'rho', 'abs', 'w'):
            a, b = np.asarray(got[i][k], dtype=np.float64), np.asarray(want[i][k], dtype=np.float64)
            assert np.allclose(a, b, rtol=1e-11, atol=1e-13 * (1.0 + np.abs(b).max(initial=0.0))), (name, i, k)
        o = offs[i - 1]
        flat[o:o + K * K], flat[o + K * K:o + K * K + K] = got[i]['A'].ravel(), got[i]['b']
        flat[o + K * K + K:o + K * K + K + 4] = got[i]['rho'], got[i]['abs'], got[i]['w'], got[i]['n']
    assert offs[-1] == sum((counts[i] + counts[0]) ** 2 + counts[i] + counts[0] if counts[i] else 0 for i in range(1, 17)) + 64
    back = rs.parse_norm_blocks(flat, counts)                          # the layout of the device output, there and back
    for i in range(1, 17):
        assert np.array_equal(back[i]['A'], got[i]['A']) and np.array_equal(back[i]['b'], got[i]['b'])
        assert (back[i]['rho'], back[i]['abs'], back[i]['w'], back[i]['n']) == tuple(float(got[i][k]) for k in ('rho', 'abs', 'w', 'n'))
    with pytest.raises(ValueError):
        rs.parse_norm_blocks(flat[:-1], counts)
    with pytest.raises(ValueError):
        rs.norm_block_offsets(counts[:-1] + [129])
    Ld, L = rs.norm_objective(got, c['n'])
    wd, w = nc.objective(c['rows'], c['lists'], c['x0'], DELTA)
    assert abs(Ld - wd) <= 1e-12 * wd and abs(L - w) <= 1e-12 * w and L <= Ld <= L + DELTA
    if name == 'shipped':                                              # the planted zero residual: w = 1 / delta exactly
        r = nc.blocks(c['rows'][3:4], c['lists'], c['x0'], mode, DELTA)[2]
        assert r['abs'] == 0.0 and r['rho'] == DELTA and r['w'] == (1.0 / DELTA if mode == nc.INV else 1.0)


@pytest.mark.parametrize('name', ['shipped', 'empty_row', 'empty_pelvis'])
def test_unit_blocks_are_the_gathered_moments(name):
    rs = _mod('regressor_solve')
    c = nc.table(name)
    M = jc.moments(c['rows'])
    got = rs.norm_blocks_reference(c['rows'], c['lists'], c['x0'], nc.UNIT, 0.0)
    for i in range(1, 17):
        pts = np.concatenate([c['lists'][i], c['lists'][0]]) if c['lists'][i].size else np.zeros(0, dtype=np.int64)
        sub = M[np.ix_(pts, pts)]
        assert np.allclose(got[i]['A'], sub, rtol=1e-12, atol=1e-13 * (1 + np.abs(sub).max(initial=0.0)))
        assert got[i]['w'] == (c['n'] if pts.size else 0) and got[i]['rho'] == got[i]['abs']


@pytest.mark.parametrize('name', ['shipped', 'empty_row', 'empty_pelvis'])
def test_gradient_against_central_differences(name):
    rs = _mod('regressor_solve')
    c = nc.table(name)
    delta, h = 1e-4, 1e-6
    lists, x = c['lists'], nc.random_feasible(np.random.RandomState(2), c['lists'])
    grads = rs.norm_gradient(rs.norm_blocks_reference(c['rows'], lists, x, nc.INV, delta), c['n'], lists)
    assert [g.size for g in grads] == [l.size for l in lists]
    scale = max(float(np.abs(g).max()) for g in grads if g.size)
    worst = 0.0
    for i in range(17):
        for e in range(min(lists[i].size, 4)):
            up, dn = [r.copy() for r in x], [r.copy() for r in x]
            up[i][e] += h
            dn[i][e] -= h
            fd = (nc.objective(c['rows'], lists, up, delta)[0] - nc.objective(c['rows'], lists, dn, delta)[0]) / (2 * h)
            worst = max(worst, abs(fd - grads[i][e]))
    print(f'{name}: worst {worst:.3e} against a largest entry of {scale:.3e}')
    assert worst <= 1e-6 * scale + 1e-16 / h


@pytest.mark.parametrize('name', ['shipped', 'empty_pelvis'])
def test_the_majoriser_lies_above(name):
    rs = _mod('regressor_solve')
    c = nc.table(name)
    lists, n = c['lists'], c['n']
    rng = np.random.RandomState(3)
    for k in range(6):
        x, y = nc.random_feasible(rng, lists), nc.random_feasible(rng, lists)
        if k % 2:
            y = [0.9 * a + 0.1 * b for a, b in zip(x, y)]
        bl = rs.norm_blocks_reference(c['rows'], lists, x, nc.INV, DELTA)
        Lx = rs.norm_objective(bl, n)[0]
        Q = Lx
        for i in range(1, 17):
            if lists[i].size:
                D = np.concatenate([y[i] - x[i], -(y[0] - x[0])])
                Q += (bl[i]['b'] @ D + 0.5 * D @ bl[i]['A'] @ D) / (n * 17)
        Ly = nc.objective(c['rows'], lists, y, DELTA)[0]
        print(f'{name} pair {k}: L_delta(y) {Ly:.9e} <= Q(y) {Q:.9e}')
        assert Ly <= Q + 1e-15
    assert abs(nc.objective(c['rows'], lists, x, DELTA)[0] - Lx) <= 1e-14


# ---- the solver ----
def test_planted_with_outliers():
    c, r = nc.table('planted'), _solved('planted')
    seq = np.asarray(r['sequence'])
    o = r['objective']
    e_mse, e_x = _worst(r['x_mse'], c['x_true']), _worst(r['x'], c['x_true'])
    print(f'planted: MPJPE {1e3 * o["start"]:.3f} -> {1e3 * o["mse"]:.3f} (MSE optimum) -> {1e3 * o["final"]:.3f} mm, gap {1e3 * r["gap"]:.2e} mm in '
          f'{r["passes"]} passes and {r["inner_iterations"]} inner steps; worst weight error {e_mse:.4f} (MSE) against {e_x:.4f}')
    assert r['converged'] and r['gap'] <= TOL * r['smoothed']['start'] and r['bound'] == r['gap'] + DELTA
    assert (np.diff(seq) <= 1e-13 * seq[:-1]).all() and len(seq) == r['passes'] - 1
    assert o['final'] <= o['mse'] + r['gap'] + DELTA
    assert o['final'] < o['mse'] < o['start']
    assert e_x < e_mse
    for x in (r['x'], r['x_mse']):
        assert all(abs(row.sum() - 1) <= 1e-12 and (row >= 0).all() for row in x)
    # the certificate against a run continued to a gap 100 times smaller
    far = _solved('planted', TOL / 100)
    assert far['converged'] and far['gap'] <= 1e-2 * TOL * far['smoothed']['start']
    assert r['smoothed']['final'] - far['smoothed']['final'] <= r['gap']
    assert o['final'] - far['objective']['final'] <= r['bound']
    # x_mse is the minimiser `solve` finds from the moments
    rs = _mod('regressor_solve')
    mse = rs.solve(jc.moments(c['rows']), c['n'], c['lists'], c['x0'], tol=1e-9, max_iter=400)
    assert _worst(mse['x'], r['x_mse']) <= 1e-5


def test_a_noise_free_planted_table_ends_at_zero():
    c, r = nc.table('clean'), _solved('clean')
    print(f'clean: MPJPE {1e3 * r["objective"]["final"]:.3e} mm, gap {1e3 * r["gap"]:.3e} mm, {r["passes"]} passes')
    assert r['objective']['final'] <= r['gap'] + DELTA
    assert _worst(r['x'], c['x_true']) <= 1e-3


@pytest.mark.parametrize('name', ['shipped', 'empty_row', 'empty_pelvis'])
def test_cases_with_shared_and_empty_rows(name):
    c, r = nc.table(name), _solved(name)
    seq = np.asarray(r['sequence'])
    print(f'{name}: {1e3 * r["objective"]["start"]:.3f} -> {1e3 * r["objective"]["final"]:.3f} mm, gap {1e3 * r["gap"]:.2e} mm, {r["passes"]} passes')
    assert r['converged'] and (np.diff(seq) <= 1e-13 * seq[:-1]).all()
    assert [row.size for row in r['x']] == [l.size for l in c['lists']]
    rng = np.random.RandomState(4)
    for _ in range(5):                                                 # no feasible point lies more than the bound below
        y = nc.random_feasible(rng, c['lists'])
        assert r['objective']['final'] <= nc.objective(c['rows'], c['lists'], y, DELTA)[1] + r['bound']
    assert abs(r['objective']['final'] - nc.objective(c['rows'], c['lists'], r['x'], DELTA)[1]) <= 1e-13


def test_the_surrogate_solver_lowers_the_surrogate():
    rs = _mod('regressor_solve')
    c = nc.table('shipped')
    bl = rs.norm_blocks_reference(c['rows'], c['lists'], c['x0'], nc.INV, DELTA)
    g = rs.norm_gradient(bl, c['n'], c['lists'])
    gap0 = rs.fw_gap(c['x0'], g)
    q = rs.solve_quadratic_blocks(bl, c['n'], c['lists'], c['x0'], rs.INNER_FRACTION * gap0)
    assert q['gap'] <= rs.INNER_FRACTION * gap0 and q['decrease'] > 0 and q['iterations'] >= 1
    assert nc.objective(c['rows'], c['lists'], q['x'], DELTA)[0] <= rs.norm_objective(bl, c['n'])[0] - q['decrease'] + 1e-15


# ---- flags, schema, declarations ----
def _ns(flags):
    return _mod('args').get_args(flags)


def test_flag_rules(tmp_path):
    rf = _mod('regressor_fit')
    vdir = tmp_path / 'meshes'
    vdir.mkdir()
    np.save(vdir / 'vertices.npy', np.zeros((1, 6890, 3), np.float32))
    ok = ['--fit_regressor', str(tmp_path / 'out'), '--fit_from', str(vdir)]
    for flags in (ok, ok + ['--fit_solve'], ok + ['--fit_solve', '--fit_solve_loss', 'mse'], ok + ['--fit_solve', '--fit_solve_loss', 'mpjpe'],
                  ok + ['--fit_solve', '--fit_solve_loss', 'mpjpe', '--fit_solve_delta_mm', '0.1', '--fit_rings', '1', '--synthetic'],
                  ok + ['--fit_solve', '--fit_solve_delta_mm', '1e-3']):
        rf.check_flags(_ns(flags))
    bad = [ok + ['--fit_solve_loss', 'mpjpe'], ok + ['--fit_solve_delta_mm', '0.1'], ['--fit_solve_loss', 'mpjpe'],
           ok + ['--fit_solve', '--fit_solve_loss', 'mpjpe', '--fit_solve_delta_mm', '0'],
           ok + ['--fit_solve', '--fit_solve_loss', 'mpjpe', '--fit_solve_delta_mm', '-1'],
           ok + ['--fit_solve', '--fit_solve_loss', 'mpjpe', '--fit_solve_delta_mm', 'inf'],
           ok + ['--fit_solve', '--fit_solve_loss', 'mpjpe', '--fit_solve_delta_mm', 'nan']]
    for flags in bad:
        with pytest.raises(ValueError):
            rf.check_flags(_ns(flags))
    with pytest.raises(SystemExit):
        _ns(ok + ['--fit_solve', '--fit_solve_loss', 'huber'])
    ns = _ns(ok)
    assert ns.fit_solve_loss == 'mse' and ns.fit_solve_delta_mm == 0.01


def test_the_norm_key_and_its_schema():
    rs, rf = _mod('regressor_solve'), _mod('regressor_fit')
    r = _solved('shipped')
    held = {'start': 0.05, 'mse': 0.04, 'final': 0.039}
    doc = json.loads(json.dumps(rs.build_norm_doc(r, 0.01, held)))
    assert sorted(doc) == sorted(rs.NORM_KEYS) and sorted(doc['objective_mm']) == sorted(rs.NORM_OBJECTIVE_KEYS)
    assert doc['delta_mm'] == 0.01 and doc['objective_mm']['final'] == pytest.approx(1000 * r['objective']['final'])
    assert doc['objective_mm']['holdout_final'] == pytest.approx(39.0) and doc['bound_mm'] == pytest.approx(doc['gap_mm'] + 0.01)
    assert doc['passes'] == r['passes'] and doc['inner_iterations'] == r['inner_iterations']
    none = rs.build_norm_doc(r, 0.01, None)
    assert none['objective_mm']['holdout_start'] is None and none['objective_mm']['holdout_final'] is None
    # mse mode writes exactly SOLVE_KEYS: build_doc knows no `norm`
    score = {'train': {'mpjpe_mm': 1.0, 'pampjpe_mm': 1.0}, 'holdout': None}
    res = {'x': None, 'loss': 2e-5, 'loss0': 1e-3, 'gap': 3e-10, 'iterations': 4, 'converged': True}
    plain = rs.build_doc('refined', {}, 5, 0, 0, [1] * 17, [1] * 17, [1] * 17, {'train_before': 1.0, 'train_after': 0.5}, res, 1e-6, score, score,
                         'p', None)
    assert sorted(plain) == sorted(rs.SOLVE_KEYS) and 'norm' not in rs.SOLVE_KEYS
    ns = _ns(['--fit_regressor', 'out', '--fit_from', 'x', '--fit_solve', '--fit_solve_loss', 'mpjpe'])
    for k in ('fit_solve_loss', 'fit_solve_delta_mm'):
        assert k in rf.flags_doc(ns)


def test_the_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'jrr.h')).read()
    for name in ('jrr_jfit_norm_bytes', 'jrr_jfit_norm_moments'):
        assert name + '(' in hdr and name in _mod('_lib').SIGNATURES
    assert 'JRR_JFIT_NORM_UNIT = 0' in hdr and 'JRR_JFIT_NORM_INV = 1' in hdr
    assert 'jnorm.hip' in _mod('build').SOURCES
    rs = _mod('regressor_solve')
    assert (rs.NORM_UNIT, rs.NORM_INV) == (0, 1)
