"""The support structures of tests/support_cases.py without a GPU: every case of tests/test_gpu_support_shapes.py has the structure that
test relies on -- the count of support vertices, the entries per row, how many rows read one vertex, the skinning influences of the
support vertices -- and the shrinking regressor loses entries under J steps, revives none and keeps all 64 vertices."""
import importlib

import numpy as np
import pytest

import support_cases as sc
from conftest import PKG_NAME


@pytest.fixture(scope='module')
def sm():
    return importlib.import_module(PKG_NAME + '.smpl_model')


def test_shipped_regressor_structure(smpl_model_np, j_h36m_np):
    """what the suite has driven the per-vertex iteration with so far (the starting point of support_cases.py's docstring)"""
    s = sc.structure(smpl_model_np, j_h36m_np)
    assert (s['nsv'], s['entries']) == (58, 62)
    assert (min(s['row_counts']), max(s['row_counts']), s['max_reads']) == (2, 5, 2)
    assert s['influences'] == {4: 58}
    assert max(s['per_joint']) == 22 and s['per_joint'].count(0) == 6
    assert (s['support'][0], s['support'][-1]) == (13, 6828)
    assert (smpl_model_np['lbs_weights'] != 0).sum(1).tolist() == [4] * sc.V


@pytest.mark.parametrize('n', [1, 2, 5, 6, 17, 64, 65, 72])
def test_vertices_spread(n):
    v = sc.vertices_spread(n, n)
    assert v.shape == (n,) and len(set(v.tolist())) == n and np.array_equal(v, np.sort(v))
    assert v.min() >= 0 and v.max() < sc.V
    assert set(sc.EDGES[:min(n, 6)]) <= set(v.tolist())
    assert np.array_equal(v, sc.vertices_spread(n, n))                      # seeded


def test_vertices_of_joint_and_wrists(smpl_model_np):
    W = smpl_model_np['lbs_weights']
    v = sc.vertices_of_joint(smpl_model_np, 64, sc.ONE_JOINT, 1)
    assert len(set(v.tolist())) == 64 and (W[v, sc.ONE_JOINT] != 0).all()
    w = sc.vertices_wrists(smpl_model_np)
    assert len(w) == 25 and ((W[w, 20] != 0) | (W[w, 21] != 0)).all()
    rest = np.setdiff1d(np.arange(sc.V), w)
    assert not (W[rest, 20] != 0).any() and not (W[rest, 21] != 0).any()


def test_regressor_layouts():
    v = sc.vertices_spread(40, 40)
    Jb = sc.regressor(v, 'blocks', 1)
    for i in range(sc.NH):
        pos = np.nonzero(Jb[i] > 0)[0]
        assert np.array_equal(pos, v[i::sc.NH]) and (Jb[i, pos] >= 0.1).all() and (Jb[i, pos] <= 0.6).all()
        neg = np.nonzero(Jb[i] < 0)[0]
        assert len(neg) == 3 and not set(neg.tolist()) & set(v.tolist())
    assert abs(Jb.clip(0).sum(1) - 1).max() > 0.05                          # not normalised
    Jd = sc.regressor(v, 'dense', 1)
    assert ((Jd > 0).sum(1) == 40).all() and np.array_equal(np.nonzero((Jd > 0).any(0))[0], v)
    scale = Jd.clip(0).sum(1)
    assert (scale > 0.49).all() and (scale < 2.01).all() and np.ptp(scale) > 0.3
    assert not (sc.regressor(v, 'dense', 1, negatives=False) < 0).any()
    J2 = sc.regressor(sc.vertices_spread(2, 2), 'blocks', 2)               # fewer vertices than rows: row i reads verts[i % n]
    assert [int(np.nonzero(r > 0)[0][0]) for r in J2] == [(0, 6889)[i % 2] for i in range(sc.NH)]
    assert np.array_equal(Jb, sc.regressor(v, 'blocks', 1))                # seeded


def test_with_influences(smpl_model_np):
    v = sc.vertices_spread(10, 3)
    counts = [1, 2, 3, 4, 6, 6, 4, 3, 2, 1]
    m = sc.with_influences(smpl_model_np, v, counts)
    W0, W1 = smpl_model_np['lbs_weights'], m['lbs_weights']
    assert W1.dtype == np.float32 and (W1[v] != 0).sum(1).tolist() == counts
    np.testing.assert_allclose(W1[v].sum(1), 1.0, atol=1e-6)
    rest = np.setdiff1d(np.arange(sc.V), v)
    assert np.array_equal(W1[rest], W0[rest]) and W0 is not W1
    for vi, k in zip(v, counts):
        kept = np.argsort(-W0[vi], kind='stable')[:min(k, 4)]
        assert (W1[vi, kept] != 0).all()                                     # its largest weights
        if k == 6:
            extra = np.setdiff1d(np.nonzero(W1[vi])[0], np.nonzero(W0[vi])[0])
            assert len(extra) == 2
            np.testing.assert_allclose(W1[vi, extra], 0.05 / 1.1, rtol=1e-6)
    assert all(m[k] is smpl_model_np[k] for k in smpl_model_np if k != 'lbs_weights')


@pytest.mark.parametrize('case', list(sc.SPEC))
def test_case_structure(smpl_model_np, case):
    c = sc.build(smpl_model_np, case)
    s = sc.structure(c['model'], c['J'], c['mask'])
    e = sc.EXPECT[case]
    assert s['nsv'] == e['nsv'] and np.array_equal(s['support'], c['support'])
    assert s['entries'] == e['entries']
    assert (min(s['row_counts']), max(s['row_counts'])) == (e['row_min'], e['row_max'])
    assert min(s['row_counts']) >= 1                                          # no row is empty after ReLU and mask
    assert s['max_reads'] == e['max_reads']
    assert s['influences'] == e['influences']
    assert (c['J'] < 0).sum() == 3 * sc.NH                                    # ReLU has something to remove
    assert c['B'] == (1 if case.endswith('_B1') else sc.B_DEFAULT)
    if sc.SPEC[case][0] == 'spread':
        assert set(sc.EDGES[:min(s['nsv'], 6)]) <= set(c['verts'].tolist())
    if case == 'masked':
        assert len(c['verts']) == 72 and int((c['mask'] == 0).any(0).sum()) == sc.MASKED_DROP
        assert ((c['J'] > 0).sum(1) == 72).all()                              # the mask, not the regressor, brings it to 64
        assert np.array_equal((c['mask'] == 0).all(0), (c['mask'] == 0).any(0))
    else:
        assert c['mask'] is None
    if c['hint'] is not None:
        assert np.array_equal(c['hint'], s['support'])
    assert (s['nsv'] <= sc.SUP_NSV) == (case != 'n65')


def test_one_joint_fills_a_joint_list(smpl_model_np):
    c = sc.build(smpl_model_np, 'one_joint')
    s = sc.structure(c['model'], c['J'])
    assert s['per_joint'][sc.ONE_JOINT] == sc.SUP_NSV == s['nsv']


def test_mask_words(smpl_model_np):
    """the bit masks of supk.h (rowm: two 32-bit words per H36M row over the support slots, colm: one word per slot) as these cases fill
    them: full words, an empty upper word, an upper word with one bit, columns with 17 bits"""
    def words(case):
        c = sc.build(smpl_model_np, case)
        P = (sc.effective(c['J'], c['mask']) > 0)[:, c['support']]
        P = np.pad(P, ((0, 0), (0, 64 - P.shape[1])))
        return P[:, :32].sum(1), P[:, 32:].sum(1), P.sum(0)
    lo, hi, col = words('n64_dense')
    assert (lo == 32).all() and (hi == 32).all() and (col == 17).all()
    lo, hi, col = words('n32')
    assert lo.sum() == 32 and (hi == 0).all()
    lo, hi, col = words('n33')
    assert lo.sum() == 32 and hi.sum() == 1
    lo, hi, col = words('n2_dense')
    assert (lo == 2).all() and (col[:2] == 17).all() and (col[2:] == 0).all()


def test_shrinking_support(smpl_model_np, sm):
    """B = 16, six iterations with a J step after each (j_lr 1e-2, no discriminator): at least 10 positive entries die, none is revived,
    every row keeps at least 4, the union of support vertices stays 64 (measured: 200 -> 174 entries, smallest row 6).  At the GPU
    test's B = 33 as well (200 -> 172, smallest row 9), and there no entry ends a J step closer to zero than 4e-5, twice the bound the
    GPU test holds J to: which entries died does not hang on rounding (measured 6.2e-5)."""
    J0 = sc.shrinking_case()
    P0 = J0 > 0
    assert int(P0.sum()) == 200 and not (J0 < 0).any() and int(P0.any(0).sum()) == sc.SUP_NSV
    for B in (16, sc.B_DEFAULT):
        r = sc.shrinking_oracle(smpl_model_np, J0, B, sm)
        P = r['positive'][-1]
        print(f'B {B}: 200 -> {[int(p.sum()) for p in r["positive"]]} entries, smallest row {int(P.sum(1).min())}, margins '
              f'{["%.1e" % m for m in r["margin"]]}')
        assert int(P0.sum()) - int(P.sum()) >= 10
        assert not any((p & ~P0).any() for p in r['positive'])
        assert all(not (q & ~p).any() for p, q in zip(r['positive'], r['positive'][1:]))      # no entry comes back between steps either
        assert int(P.sum(1).min()) >= 4
        assert int(P.any(0).sum()) == sc.SUP_NSV
        if B == sc.B_DEFAULT:
            assert min(r['margin']) > 4e-5, r['margin']
