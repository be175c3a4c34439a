"""The prices of all mesh vertices in the regressor solve (`--fit_solve --fit_grow R`), host side: numpy float64, no GPU.

The device pass (include/jrr.h, jrr_jfit_price) is restated by regressor_solve.price_reference; here the restatement is tested against
the DEFINITION -- central differences of the loss in a dense (17, 6890) weight array -- and against the gradients the solve already
uses, and the column generation (global_gap, grow_select, grow) against hand-made cases and a table whose optimum is planted far from
the initial support."""
import json
import os

import numpy as np
import pytest

import jprice_cases as C
from conftest import PKG_NAME, ROOT

import importlib


def _mod(name):
    return importlib.import_module(PKG_NAME + '.' + name)


NJ, NV = 17, 6890
EDGE = (0, 6879, 6880, 6889)


def _small(n=6, seed=5, empty_row=None, empty_pelvis=False):
    """n random meshes, ground truth of the size of a body, lists of 1 .. 6 vertices that avoid EDGE, random weights on the simplex"""
    rng = np.random.default_rng(seed)
    verts = rng.normal(0.0, 0.4, (n, NV, 3)).astype(np.float32)
    gt = rng.normal(0.0, 300.0, (n, NJ, 3)).astype(np.float32)
    gt[:, 0] = 0.0
    cands, x = [], []
    for i in range(NJ):
        k = 0 if (i == empty_row or (i == 0 and empty_pelvis)) else 1 + (i % 6)
        v = np.sort(rng.choice(np.arange(1, 6879), k, replace=False))
        w = rng.uniform(0.1, 1.0, k)
        cands.append(v)
        x.append(w / w.sum() if k else w)
    return verts, gt, cands, x


def _dense(cands, x):
    W = np.zeros((NJ, NV))
    for i, (v, w) in enumerate(zip(cands, x)):
        W[i, v] = w
    return W


@pytest.mark.parametrize('case', ['full', 'empty_row', 'empty_pelvis'])
@pytest.mark.parametrize('mode', [0, 1])
def test_prices_are_the_gradient_of_the_loss_in_a_dense_weight_array(case, mode):
    """central differences of the loss at unlisted vertices (the corners of the vertex range among them), at listed ones, in row 0 and in
    joint rows.  MSE is a quadratic, so the central difference is exact up to rounding at any step: rtol 1e-9.  NORM: step 1e-6, rtol 1e-6."""
    rs = _mod('regressor_solve')
    verts, gt, cands, x = _small(empty_row=9 if case == 'empty_row' else None, empty_pelvis=case == 'empty_pelvis')
    delta = 1e-5
    n = verts.shape[0]
    out = rs.price_reference(verts, gt, cands, x, mode, delta if mode else 0.0)
    g = rs.price_gradients(out, n, cands, mode)
    active = [v.size > 0 for v in cands]
    W = _dense(cands, x)
    h, rtol = (0.25, 1e-9) if mode == 0 else (1e-6, 1e-6)
    loss = lambda Wd: C.dense_loss(verts, gt, Wd, mode, delta if mode else 0.0, active)
    assert abs(loss(W) - rs.price_loss(out, n, mode)) <= 1e-12 * loss(W)
    rows = [i for i in (0, 1, 8, 9, 16) if active[i]]
    for i in rows:
        for u in EDGE + (int(cands[i][0]), 3000):
            Wp, Wm = W.copy(), W.copy()
            Wp[i, u] += h
            Wm[i, u] -= h
            fd = (loss(Wp) - loss(Wm)) / (2 * h)
            assert abs(fd - g[i, u]) <= rtol * abs(g[i, u]), (i, u, fd, g[i, u])
    for i in range(NJ):
        if not active[i]:
            assert not g[i].any()                                   # a row without entries has no parameters: zeros


def test_prices_at_listed_vertices_are_the_gradients_of_the_solve():
    rs = _mod('regressor_solve')
    for kw in ({}, {'empty_row': 4}, {'empty_pelvis': True}):
        verts, gt, cands, x = _small(n=9, seed=8, **kw)
        n = verts.shape[0]
        M, lists, cols = C.moments_of(verts, gt, cands)
        _, grads = rs.loss_from_moments(M, n, lists, x)
        g = rs.price_gradients(rs.price_reference(verts, gt, cands, x, rs.PRICE_MSE, 0.0), n, cands, rs.PRICE_MSE)
        for i in range(NJ):
            np.testing.assert_allclose(g[i, cands[i]], grads[i], rtol=1e-10, atol=0)
        delta = 2e-5
        rows = np.concatenate([verts[:, cols], gt], 1)
        blocks = rs.norm_blocks_reference(rows, lists, x, rs.NORM_INV, delta)
        grads = rs.norm_gradient(blocks, n, lists)
        out = rs.price_reference(verts, gt, cands, x, rs.PRICE_NORM, delta)
        g = rs.price_gradients(out, n, cands, rs.PRICE_NORM)
        for i in range(NJ):
            np.testing.assert_allclose(g[i, cands[i]], grads[i], rtol=1e-10, atol=0)
        # the scalars: sum rho, sum |r| and the samples are the blocks'
        tail = out[16 * NV:].reshape(16, 4)
        for i in range(1, NJ):
            b = blocks[i]
            np.testing.assert_allclose(tail[i - 1, 1:], [b['rho'], b['abs'], b['n']], rtol=1e-13)


def test_price_reference_refuses_what_the_device_refuses():
    rs = _mod('regressor_solve')
    verts, gt, cands, x = _small(n=2)
    for mode, delta in ((2, 0.0), (0, -1.0), (0, np.nan), (1, 0.0), (1, np.inf)):
        with pytest.raises(ValueError):
            rs.price_reference(verts, gt, cands, x, mode, delta)
    bad = [c.copy() for c in cands]
    bad[3] = np.array([5, 5])
    with pytest.raises(ValueError):
        rs.price_reference(verts, gt, bad, [np.ones(c.size) / max(c.size, 1) for c in bad], 0, 0.0)
    bad[3] = np.array([NV])
    with pytest.raises(ValueError):
        rs.price_reference(verts, gt, bad, [np.ones(c.size) / max(c.size, 1) for c in bad], 0, 0.0)
    with pytest.raises(ValueError):
        rs.price_reference(verts, gt, [np.zeros(0, dtype=np.int64)] * NJ, [np.zeros(0)] * NJ, 0, 0.0)


@pytest.mark.parametrize('empty_pelvis', [False, True])
@pytest.mark.parametrize('mode', [0, 1])
def test_the_restatement_in_two_orders_stays_within_the_device_bound(mode, empty_pelvis):
    """the condition of the GPU comparison (tests/test_gpu_regressor_grow.py): price_reference is itself a rounded float64 sum, so the
    bound the device is held to must be far above what another ORDER of the same float64 sum costs on the inputs of that test -- the
    meshes permuted, every list reversed.  Under 5 % of the bound, so the reference takes none of the device's room that matters."""
    rs = _mod('regressor_solve')
    for batch in (5, 130):
        verts, gt, cands, x = C.float_case(batch, empty_pelvis)
        delta = 1e-5 if mode else 0.0
        one = rs.price_reference(verts, gt, cands, x, mode, delta)
        p = np.random.default_rng(batch).permutation(batch)
        two = rs.price_reference(verts[p], gt[p], [c[::-1] for c in cands], [w[::-1] for w in x], mode, delta)
        bS, bs = C.price_bound(verts, gt, cands, x, mode, delta)
        (S1, t1), (S2, t2) = C.split_out(one), C.split_out(two)
        live = bS > 0
        assert not S1[~live].any() and not S2[~live].any()         # the empty row
        assert (np.abs(S1 - S2)[live] <= 0.05 * bS[live]).all()
        assert (np.abs(t1[:, :3] - t2[:, :3]) <= 0.05 * bs).all() and np.array_equal(t1[:, 3], t2[:, 3])


# ---- the global gap and the selection ------------------------------------------------------------------------------------------------
def test_global_gap_contains_the_listed_gap():
    rs = _mod('regressor_solve')
    verts, gt, cands, x = _small(n=5, seed=2, empty_row=7)
    n = verts.shape[0]
    g = rs.price_gradients(rs.price_reference(verts, gt, cands, x, 0, 0.0), n, cands, 0)
    listed = rs.fw_gap(x, [g[i, cands[i]] for i in range(NJ)])
    gap, lam, low = rs.global_gap(g, cands, x, None)
    assert gap >= listed > 0
    assert low[7] == 0.0 and lam[7] == 0.0 and (low <= 0).all()
    only = np.zeros((NJ, NV))
    for i, v in enumerate(cands):
        only[i, v] = 1.0
    gap_l, lam_l, _ = rs.global_gap(g, cands, x, only)
    assert gap_l == pytest.approx(listed, rel=1e-13) and np.array_equal(lam, lam_l)
    # an eligible set that forgets a listed entry still contains it: a listed entry is a vertex of its row
    assert rs.global_gap(g, cands, x, np.zeros((NJ, NV)))[0] == gap_l
    for i in range(NJ):
        if cands[i].size:
            assert lam[i] == pytest.approx(float(g[i, cands[i]] @ x[i]), rel=1e-15)
            assert low[i] == pytest.approx(g[i].min() - lam[i], rel=1e-15)


def _hand():
    """row 0 empty, row 1 = {10: 0.5, 20: 0.5, 30: 0}, row 2 = {40: 1}, the other rows one vertex each; g zero but where the cases set it"""
    cands = [np.zeros(0, dtype=np.int64), np.array([10, 20, 30]), np.array([40])] + [np.array([100 + i]) for i in range(3, NJ)]
    x = [np.zeros(0), np.array([0.5, 0.5, 0.0]), np.array([1.0])] + [np.array([1.0]) for _ in range(3, NJ)]
    return cands, x, np.zeros((NJ, NV))


def test_grow_select_ties_drops_and_order():
    rs = _mod('regressor_solve')
    cands, x, g = _hand()
    g[1, [10, 20]] = 1.0                                            # lambda_1 = 1
    g[1, 30] = 2.0
    g[1, [7, 5, 9]] = -3.0                                          # a tie of three
    g[1, 6] = -4.0
    g[1, 8] = 0.5                                                   # reduced cost -0.5
    g[1, 11] = 1.0                                                  # reduced cost 0: not strictly below
    g[2, 40] = -1.0                                                 # lambda_2 = -1: nothing lies below
    for i in range(3, NJ):
        g[i, 100 + i] = -1.0
    g[1, 12:] = np.where(g[1, 12:] == 0.0, 1.0, g[1, 12:])          # the rest of row 1 at reduced cost 0
    g[1, :5] = 1.0
    sel = rs.grow_select(g, cands, x, None, 3)
    assert sel['dropped'] == [0, 1] + [0] * 15 and sel['added'] == [0, 3] + [0] * 15 and sel['capped'] is False
    assert sel['cands'][1].tolist() == [5, 6, 7, 10, 20]            # 30 dropped (weight exactly 0); -4 first, then the tie's lower vertices
    assert sel['x'][1].tolist() == [0.0, 0.0, 0.0, 0.5, 0.5]
    assert sel['cands'][0].size == 0 and sel['cands'][2].tolist() == [40]
    sel = rs.grow_select(g, cands, x, None, 128)
    assert sel['cands'][1].tolist() == [5, 6, 7, 8, 9, 10, 20] and sel['added'][1] == 5       # everything strictly below 0, nothing else
    # eligibility: a masked vertex is never added
    el = np.ones((NJ, NV))
    el[1, 6] = 0.0
    sel = rs.grow_select(g, cands, x, el, 2)
    assert sel['cands'][1].tolist() == [5, 7, 10, 20]
    # a zero-weight entry with a negative reduced cost is dropped and may come straight back: drops come first
    g[1, 30] = -5.0
    sel = rs.grow_select(g, cands, x, None, 1)
    assert sel['dropped'][1] == 1 and sel['cands'][1].tolist() == [10, 20, 30] and sel['x'][1].tolist() == [0.5, 0.5, 0.0]


def test_grow_select_row_cap_and_union_cap():
    rs = _mod('regressor_solve')
    cands, x, g = _hand()
    # the row cap: row 1 holds 126 positive entries and wants 5 more
    v = np.arange(1000, 1126)
    cands[1], x[1] = v, np.full(126, 1.0 / 126)
    g[1, :5] = -1.0
    sel = rs.grow_select(g, cands, x, None, 5)
    assert sel['added'][1] == 2 and sel['cands'][1].size == 128 and sel['cands'][1][:2].tolist() == [0, 1] and sel['capped'] is True
    sel = rs.grow_select(g, cands, x, None, 2)
    assert sel['added'][1] == 2 and sel['capped'] is False
    # the union cap: 16 rows of 128 different vertices and row 0 with 127 fill 2175 of the 2176 columns
    cands = [np.arange(128 * i, 128 * i + (127 if i == 0 else 128)) for i in range(NJ)]
    x = [np.full(c.size, 1.0 / c.size) for c in cands]
    g = np.zeros((NJ, NV))
    g[0, 3000] = -2.0                                               # a new column: fits
    g[0, 128] = -1.0                                                # row 1's vertex, in the union already -- but row 0 is full by then
    sel = rs.grow_select(g, cands, x, None, 2)
    assert sel['added'][0] == 1 and 3000 in sel['cands'][0] and sel['capped'] is True
    cands[0] = cands[0][:100]
    x[0] = np.full(100, 0.01)
    g[0, 3001] = -1.5
    sel = rs.grow_select(g, cands, x, None, 3)                      # 2148 + 28 columns are free: 3000 and 3001 fit, 128 is shared
    assert sel['added'][0] == 3 and sel['capped'] is False
    filler = np.arange(4000, 4027)                                  # 27 more columns in row 0: the union stands at 2175
    cands[0] = np.concatenate([cands[0], filler])
    x[0] = np.full(127, 1.0 / 127)
    sel = rs.grow_select(g, cands, x, None, 3)
    assert sel['added'][0] == 1 and sel['cands'][0].size == 128 and 3000 in sel['cands'][0] and sel['capped'] is True
    # 17 rows of at most 128 entries: the union of the lists cannot pass 17 * 128 = 2176, the columns the state of the fit holds
    assert np.unique(np.concatenate(sel['cands'])).size == rs.UNION_CAP


# ---- the planted table ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def planted():
    rs = _mod('regressor_solve')
    verts, gt, cands0, x0, where, _ = C.planted_table()
    solve_fn, price_fn = C.host_solver(verts, gt)
    res = rs.grow(solve_fn, price_fn, cands0, x0, 1e-6, 12, 8, None)
    return verts, gt, cands0, x0, where, res, solve_fn, price_fn


def test_planted_table_converges_over_the_whole_mesh(planted):
    verts, gt, cands0, x0, where, res, _, _ = planted
    rounds = res['rounds']
    print([(r['round'], sum(r['candidates']), r['loss'], r['global_gap']) for r in rounds])
    assert res['global_converged'] and len(rounds) <= 13 and res['global_gap'] <= 1e-6 * res['loss0']
    assert [r['round'] for r in rounds] == list(range(len(rounds)))
    for a, b in zip(rounds, rounds[1:]):
        assert b['loss'] <= a['loss']                               # warm-started at the previous weights: the loss never rises
    for r in rounds:
        assert sorted(r) == sorted(_mod('regressor_solve').GROW_ROUND_KEYS)
        assert r['loss'] <= r['global_gap']                         # the optimum is 0: this is the certificate itself
        assert r['gap'] <= r['global_gap'] + 1e-15 and max(r['candidates']) <= 128 and all(m <= 0 for m in r['min_reduced'])
    assert rounds[0]['loss'] > 1e-3 and rounds[0]['gap'] <= 1e-6 * res['loss0'] < rounds[0]['global_gap']    # what the listed gap cannot see
    for i in range(NJ):
        for p in where[i]:
            k = np.flatnonzero(res['cands'][i] == p)
            assert k.size == 1 and res['x'][i][k[0]] > 0, (i, p)
    for v, w in zip(res['cands'], res['x']):
        assert (np.diff(v) > 0).all() and w.sum() == pytest.approx(1.0, abs=1e-12) and (w >= 0).all()


def test_zero_rounds_is_the_plain_solve(planted):
    rs = _mod('regressor_solve')
    verts, gt, cands0, x0, _, _, solve_fn, price_fn = planted
    res = rs.grow(solve_fn, price_fn, cands0, x0, 1e-6, 0, 8, None)
    plain = solve_fn(cands0, x0)
    assert len(res['rounds']) == 1 and not res['global_converged']
    for a, b, c, d in zip(res['x'], plain['x'], res['cands'], cands0):
        assert np.array_equal(a, b) and np.array_equal(c, d)
    assert res['rounds'][0]['added'] == [0] * NJ and res['rounds'][0]['loss'] == plain['loss']
    with pytest.raises(ValueError):
        rs.grow(solve_fn, price_fn, cands0, x0, 1e-6, -1, 8, None)
    with pytest.raises(ValueError):
        rs.grow(solve_fn, price_fn, cands0, x0, 1e-6, 1, 0, None)


# ---- the command surface ---------------------------------------------------------------------------------------------------------------
def _ns(flags):
    return _mod('args').get_args(flags)


def test_flag_rules(tmp_path):
    rf = _mod('regressor_fit')
    vdir = tmp_path / 'meshes'
    vdir.mkdir()
    np.save(vdir / 'vertices.npy', np.zeros((1, 6890, 3), np.float32))
    ok = ['--fit_regressor', str(tmp_path / 'out'), '--fit_from', str(vdir)]
    for flags in (ok + ['--fit_solve', '--fit_grow', '0'], ok + ['--fit_solve', '--fit_grow', '6', '--fit_grow_add', '128'],
                  ok + ['--fit_solve', '--fit_grow', '2', '--fit_grow_add', '1', '--fit_rings', '1', '--synthetic'],
                  ok + ['--fit_solve', '--fit_grow', '2', '--fit_solve_loss', 'mpjpe'], ok + ['--fit_solve']):
        rf.check_flags(_ns(flags))
    bad = [ok + ['--fit_grow', '2'],                                 # needs --fit_solve
           ok + ['--fit_solve', '--fit_grow', '-1'], ok + ['--fit_solve', '--fit_grow', '2', '--fit_grow_add', '0'],
           ok + ['--fit_solve', '--fit_grow', '2', '--fit_grow_add', '129'], ok + ['--fit_grow_add', '4'],
           ok + ['--fit_solve', '--fit_grow_add', '4'], ['--fit_grow', '1'], ['--fit_solve', '--fit_grow', '1']]
    for flags in bad:
        with pytest.raises(ValueError):
            rf.check_flags(_ns(flags))
    ns = _ns(ok)
    assert ns.fit_grow is None and ns.fit_grow_add == 8


def test_the_library_surface():
    hdr = open(os.path.join(ROOT, 'include', 'jrr.h')).read()
    for name in ('jrr_jfit_price_bytes', 'jrr_jfit_price'):
        assert name + '(' in hdr and name in _mod('_lib').SIGNATURES
    assert 'JRR_JFIT_PRICE_DOUBLES = 16 * 6890 + 16 * 4' in hdr and 'JRR_JFIT_PRICE_MSE = 0, JRR_JFIT_PRICE_NORM = 1' in hdr
    assert hdr.index('jrr_jfit_norm_moments(') < hdr.index('jrr_jfit_price_bytes(')
    assert 'jprice.hip' in _mod('build').SOURCES
    rs = _mod('regressor_solve')
    assert rs.PRICE_DOUBLES == 16 * 6890 + 64 and (rs.PRICE_MSE, rs.PRICE_NORM) == (0, 1)


def test_solve_json_without_the_flag_is_unchanged():
    rs = _mod('regressor_solve')
    assert rs.SOLVE_KEYS == ('layout_version', 'source', 'flags', 'rows', 'rings', 'support', 'loss', 'gap', 'tol', 'iterations', 'converged',
                             'initial', 'final', 'checkpoint', 'j_regressor_init')
    score = {'train': {'mpjpe_mm': 1.0, 'pampjpe_mm': 1.0}, 'holdout': None}
    res = {'x': None, 'loss': 0.5, 'loss0': 1.0, 'gap': 1e-9, 'iterations': 3, 'converged': True}
    doc = rs.build_doc('vertices', {}, 5, 0, 0, [1] * 17, [1] * 17, [1] * 17, {'train_before': 1.0, 'train_after': 0.5}, res, 1e-6, score, score,
                       'p', None)
    assert sorted(doc) == sorted(rs.SOLVE_KEYS)
    rec = {'round': 0, 'candidates': [1] * 17, 'support': [1] * 17, 'loss': 0.5, 'gap': 1e-9, 'global_gap': 1e-3, 'added': [0] * 17,
           'dropped': [0] * 17, 'min_reduced': [0.0] * 17, 'capped': False}
    g = rs.build_grow_doc({'rounds': [rec], 'global_gap': 1e-3, 'global_converged': False}, add=8, max_rounds=6, eligible=17 * 6890)
    assert sorted(g) == sorted(rs.GROW_KEYS) and g['eligible'] == 117130 and g['rounds'][0]['round'] == 0
    json.dumps(g)
