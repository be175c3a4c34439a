"""The per-vertex error without a GPU: the float32 host restatement of include/jrr.h (tests/vertex_error_cases.py) against the
reference's values (tests/golden/g12_vertex_error.npz) and against float64, the derivation of the report from a hand-made int64 table,
the markdown, what `--eval_pve` refuses, and the part labels of the synthetic body.

Bounds.  The GPU tests hold the kernel to vertex_error_cases.bound = max(floor, 1.5 x the restatement's own distance from float64).
Here the restatement itself is held to float64 by the precision of float32 (FORMAT below), per vertex and -- a mean over three
vertices averages nothing away -- per pose alike, and to the reference's values by FORMAT plus the reference's own distance from
float64 (the floors, printed by tests/golden/make_golden_pve.py)."""
import importlib
import json
import os

import numpy as np
import pytest

import vertex_error_cases as vc
from conftest import PKG_NAME, ROOT

F = np.float32
# an aligned distance is formed from root-centred coordinates below 2 m (half an ulp there: 2^-24 m = 6e-8 m) by about a dozen rounded
# operations on terms of that size (the centring, three products and two sums per row of R, the scale, the translation, the
# difference), on top of the roundings of the nine entries of R, the scale and t (another dozen half-ulps on terms of up to 1.5 m):
# 24 x 6e-8 m x 1.5 = 2.1e-6 m if every one of them pointed the same way
FORMAT = 24 * 2.0 ** -24 * 1.5


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


@pytest.fixture(scope='module')
def g12():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'g12_vertex_error.npz')) as z:
        return {k: z[k] for k in z.files}


# ---- 1. the restatement ----
@pytest.mark.parametrize('n_verts', vc.G12_VERTS)
def test_restatement_against_the_reference_and_float64(g12, n_verts):
    for name in vc.FAMILIES:
        pred, gt, rp, rg = vc.family_case(name, n_verts)
        d, e, pve, pa = vc.restate(pred, gt, rp, rg)
        d64, e64, pve64, pa64 = vc.evaluate64(pred, gt, rp, rg)
        sub = vc.subset(n_verts)
        dv, dp = max(vc.dist(d, d64), vc.dist(e, e64)), max(vc.dist(pve, pve64), vc.dist(pa, pa64))
        rv = max(vc.dist(d[:, sub], g12[f'{name}_{n_verts}_d']), vc.dist(e[:, sub], g12[f'{name}_{n_verts}_e']))
        rp_ = max(vc.dist(pve, g12[f'{name}_{n_verts}_pve']), vc.dist(pa, g12[f'{name}_{n_verts}_pa']))
        print(f'{name} {n_verts}: restatement against float64 {dv:.3e} / {dp:.3e} m (per vertex / per pose), against the reference {rv:.3e} / {rp_:.3e} m')
        assert d.dtype == F and e.dtype == F and pve.dtype == F and pa.dtype == F and np.isfinite(e).all()
        assert dv <= FORMAT and dp <= FORMAT
        assert rv <= FORMAT + vc.FLOOR_VERTEX and rp_ <= FORMAT + vc.FLOOR_POSE      # each within its own distance of float64
        if name == 'constant_target':
            assert not e.any() and not pa.any()                             # exactly 0
        if name == 'similarity_copy':
            assert pa.max() <= FORMAT                                       # an exact copy aligns to nothing but rounding


def test_restatement_degenerate_shapes():
    pred, gt, rp, rg = vc.family_case('body', 65)
    const = pred.copy()
    const[:] = const[:, [3], :]
    d, e, pve, pa = vc.restate(const, gt, rp, rg)
    assert np.isfinite(d).all() and np.isfinite(pve).all() and np.isnan(e).all() and np.isnan(pa).all()      # a constant pred: NaN in e only
    d, e, pve, pa = vc.restate(pred[:, :1], gt[:, :1], rp, rg)
    assert d.shape == (4, 1) and np.isfinite(d).all() and np.isnan(e).all() and np.isnan(pa).all()          # one vertex likewise
    bad = pred.copy()
    bad[1, 7, 2] = np.nan
    d, e, pve, pa = vc.restate(bad, gt, rp, rg)
    assert np.isnan(pve[1]) and np.isnan(pa[1]) and np.isfinite(pve[[0, 2, 3]]).all() and int(np.isnan(d).sum()) == 1
    far = pred.copy()
    far[2, 0, 0] = F(2.0e3)
    assert np.isnan(vc.restate(far, gt, rp, rg)[2][2])                                                   # a distance above the cap: no mean
    # the means are exact integer sums: any order of the vertices gives the same bits
    perm = np.random.RandomState(0).permutation(65)
    a, b = vc.restate(pred, gt, rp, rg), vc.restate(pred[:, perm], gt[:, perm], rp, rg)
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert vc.fixed(np.array([0.5, 2.0 ** -25, 3 * 2.0 ** -25, np.nan, 1.0e3, 999.0], dtype=F)).tolist() == [1 << 23, 0, 2, 0, 0, 999 << 24]


# ---- 2. the tables, the derivation, the markdown ----
def _hand_made():
    """two groups, three parts (one of them empty) and an out-of-range label, five poses: one ignored, one NaN"""
    rs = np.random.RandomState(3)
    n = 6
    d = np.abs(rs.randn(5, n) * 0.05).astype(F)
    e = np.abs(rs.randn(5, n) * 0.02).astype(F)
    d[3, 2] = np.nan
    group = np.array([0, 1, 1, 1, -1], dtype=np.int32)
    part = np.array([0, 0, 2, 2, 2, 7], dtype=np.int32)
    return d, e, vc.pose_mean(d), vc.pose_mean(e), group, part


def test_accumulate_and_derive_from_a_hand_made_table():
    vr = _mod('vertex_report')
    d, e, pve, pa, group, part = _hand_made()
    table, table_v = vc.accumulate(d, e, pve, pa, group, 2, part, 3)
    rows = table[:-2].reshape(2, vc.ROW)
    assert (vr.ROW, vr.TRAILER, vr.COUNT, vr.BAD, vr.SUM, vr.SUM_PA, vr.HIST, vr.HIST_PA, vr.PART, vr.PART_PA, vr.BINS) == \
        (vc.ROW, vc.TRAILER, vc.COUNT, vc.BAD, vc.SUM, vc.SUM_PA, vc.HIST, vc.HIST_PA, vc.PART, vc.PART_PA, vc.BINS)
    assert rows[:, vc.COUNT].tolist() == [1, 2] and rows[:, vc.BAD].tolist() == [0, 1] and table[-2:].tolist() == [1, 0]
    assert rows[:, vc.HIST:vc.HIST + vc.BINS].sum(1).tolist() == [1, 2] and not rows[:, vc.PART + 1].any() and not rows[:, vc.PART + 3:vc.PART + 32].any()
    assert np.array_equal(table_v[0], vc.fixed(d[:3]).sum(0)) and np.array_equal(table_v[1], vc.fixed(e[:3]).sum(0))      # the NaN pose adds nothing
    doc = vr.derive(table, table_v, ['a', 'b'], part, 3)
    assert doc['ignored'] == 1 and doc['all']['n'] == 3 and doc['all']['n_bad'] == 1 and doc['groups']['a']['n'] == 1
    assert abs(doc['all']['pve_mm'] - float(pve[:3].astype(np.float64).mean()) * 1000) <= 1000 * 2.0 ** -25
    assert abs(doc['groups']['b']['pa_pve_mm'] - float(pa[1:3].astype(np.float64).mean()) * 1000) <= 1000 * 2.0 ** -25
    want = float(d[:3, 2:5].astype(np.float64).mean()) * 1000
    assert abs(doc['all']['pve_per_part_mm']['R_Hip'] - want) <= 1e-4 and doc['all']['pve_per_part_mm']['L_Hip'] is None
    assert doc['parts'] == {'Pelvis': 2, 'L_Hip': 0, 'R_Hip': 3}
    assert doc['per_vertex_mm'].shape == (2, 6) and doc['per_vertex_mm'].dtype == F
    assert np.allclose(doc['per_vertex_mm'][0], d[:3].astype(np.float64).mean(0) * 1000, atol=1e-4)
    lo, hi = sorted(float(v) * 1000 for v in pve[1:3])
    assert int(lo) <= doc['groups']['b']['pve_median_mm'] <= int(lo) + 1 and doc['groups']['b']['pve_p90_mm'] <= int(hi) + 1
    # a table without a counted pose, a wrong size, a pose with a group outside
    empty = vr.derive(np.zeros(vc.ROW + 2, dtype=np.int64), np.zeros((2, 6), dtype=np.int64), ['all'])
    assert empty['all']['pve_mm'] is None and np.isnan(empty['per_vertex_mm']).all() and empty['parts'] is None
    with pytest.raises(ValueError, match='372 int64 expected for 1 groups'):
        vr.derive(table, table_v, ['all'])
    table[-1] = 2
    with pytest.raises(RuntimeError, match='2 poses carried a group id outside'):
        vr.derive(table, table_v, ['a', 'b'], part, 3)


def test_files_and_markdown(tmp_path):
    vr = _mod('vertex_report')
    d, e, pve, pa, group, part = _hand_made()
    table, table_v = vc.accumulate(d, e, pve, pa, group, 2, part, 3)
    out = str(tmp_path / 'out')
    doc = vr.write(out, vr.derive(table, table_v, ['a', 'b'], part, 3), ['a', 'b'], 'action', 'vertices', ('J.npy', '0123456789abcdef'))
    assert sorted(os.listdir(out)) == ['pve.json', 'pve.md', 'pve_per_vertex.npy']
    assert vr.load(out) == json.loads(json.dumps(doc, default=str)) and np.load(os.path.join(out, 'pve_per_vertex.npy')).shape == (2, 6)
    md = open(os.path.join(out, 'pve.md'), encoding='utf-8').read()
    assert md.startswith('# Per-vertex error (vertices, groups by action)') and '| group | n | bad | PVE |' in md
    assert f'| all | 3 | 1 | {doc["data"]["all"]["pve_mm"]:.2f} |' in md and '| L_Hip | 0 | - | - |' in md and '| R_Hip | 3 |' in md
    assert '1 samples were not scored' in md and 'pve_per_vertex.npy' in md
    assert vr.summary_line(doc).startswith('per-vertex error, mm: PVE ') and '(n 3, bad 1)' in vr.summary_line(doc)
    with open(os.path.join(out, 'pve.json'), 'w') as f:
        json.dump(dict(doc, layout_version=0), f, default=str)
    with pytest.raises(ValueError, match='layout version 0'):
        vr.load(out)


# ---- 3. flags and files ----
def test_flags_and_what_eval_pve_refuses(tmp_path):
    vr, a, er = _mod('vertex_report'), _mod('args'), _mod('eval_report')
    ns = a.get_args([])
    assert ns.eval_pve is False and ns.eval_pve_parts is False
    vr.check_flags(ns)
    for flags, msg in ((['--eval_pve'], '--eval_pve needs --eval_vertices'), (['--eval_pve', '--eval_vertices', 'd'], '--eval_pve needs --eval_vertices'),
                       (['--eval_pve', '--eval_report', 'o'], '--eval_pve needs --eval_vertices'), (['--eval_pve_parts'], '--eval_pve_parts needs --eval_pve')):
        with pytest.raises(ValueError, match=msg):
            vr.check_flags(a.get_args(flags))
    vr.check_flags(a.get_args(['--eval_pve', '--eval_pve_parts', '--eval_vertices', 'd', '--eval_report', 'o']))
    assert 'eval_pve' not in vr.flags_doc(vars(ns)) and 'eval_pve_parts' not in vr.flags_doc(vars(ns)) and 'eval_report' in vr.flags_doc(vars(ns))
    # the file
    d = str(tmp_path / 'meshes')
    os.makedirs(d)
    np.save(os.path.join(d, 'vertices.npy'), np.zeros((3, 6890, 3), dtype=F))
    np.save(os.path.join(d, 'gt_j3d.npy'), np.ones((3, 17, 3), dtype=F))
    with pytest.raises(FileNotFoundError, match='gt_vertices.npy is missing'):
        vr.open_gt_vertices(d, 3)
    for arr, msg in ((np.zeros((2, 6890, 3), dtype=F), r'gt_vertices.npy: \(3,6890,3\) expected for 3 meshes, got \(2, 6890, 3\)'),
                     (np.zeros((3, 6890, 3), dtype=np.float64), 'gt_vertices.npy: float32 expected, got float64'),
                     (np.zeros((3, 431, 3), dtype=F), r'gt_vertices.npy: \(3,6890,3\) expected')):
        np.save(os.path.join(d, 'gt_vertices.npy'), arr)
        with pytest.raises(ValueError, match=msg):
            vr.open_gt_vertices(d, 3)
    withnan = np.zeros((3, 6890, 3), dtype=F)
    withnan[1] = np.nan
    np.save(os.path.join(d, 'gt_vertices.npy'), withnan)
    assert isinstance(vr.open_gt_vertices(d, 3), np.memmap)                  # NaN rows are allowed: counted as bad
    # through the driver: refused before anything is launched (no device is touched: the errors come first)
    saved = a._LazyArgs._ns
    try:
        os.remove(os.path.join(d, 'gt_vertices.npy'))
        a._LazyArgs._ns = a.get_args(['--eval_vertices', d, '--eval_report', str(tmp_path / 'o'), '--eval_pve', '--synthetic'])
        with pytest.raises(FileNotFoundError, match='gt_vertices.npy is missing'):
            er.evaluate_vertices()
        a._LazyArgs._ns = a.get_args(['--eval_vertices', d, '--regressor_report', str(tmp_path / 'o'), '--eval_pve', '--synthetic'])
        with pytest.raises(ValueError, match='--eval_pve needs --eval_vertices DIR .* and --eval_report OUT'):
            er.evaluate_vertices()
        np.save(os.path.join(d, 'gt_vertices.npy'), withnan)
        a._LazyArgs._ns = a.get_args(['--eval_vertices', d, '--eval_report', str(tmp_path / 'o'), '--eval_pve', '--eval_pve_parts', '--smpl_dir',
                                      str(tmp_path / 'no_model')])
        with pytest.raises(ValueError, match='--eval_pve_parts needs the body model'):
            er.evaluate_vertices()
    finally:
        a._LazyArgs._ns = saved
    assert not os.path.exists(str(tmp_path / 'o'))


# ---- 4. part labels ----
def test_part_labels_on_the_synthetic_body(smpl_model_np):
    vr = _mod('vertex_report')
    W = smpl_model_np['lbs_weights']
    lab = vr.part_labels(W)
    assert lab.shape == (6890,) and lab.dtype == np.int32 and lab.min() >= 0 and lab.max() < 24
    assert np.array_equal(W[np.arange(6890), lab], W.max(1))
    assert vr.part_labels(np.array([[0.5, 0.5, 0.0], [0.1, 0.45, 0.45], [0.0, 0.0, 1.0]])).tolist() == [0, 1, 2]      # ties: the lowest index
    assert len(vr.PART_NAMES) == 24 and vr.part_names(3) == ['Pelvis', 'L_Hip', 'R_Hip'] and vr.part_names(26)[-1] == 'part_25'
    with pytest.raises(ValueError, match='skinning weights'):
        vr.part_labels(np.zeros((10, 40)))


def test_symbol_declared_bound_and_documented():
    hdr = open(os.path.join(ROOT, 'include', 'jrr.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    lib_mod, eng, b = _mod('_lib'), _mod('engine'), _mod('build')
    assert 'jrr_vertex_error(' in hdr and 'jrr_vertex_error' in lib_mod.SIGNATURES and '`jrr_vertex_error`' in doc
    assert len(lib_mod.SIGNATURES['jrr_vertex_error'][1]) == 17 and 'pve.hip' in b.SOURCES and 'procfit.h' in b.HEADERS
    assert (eng.PVE_ACC_ROW, eng.PVE_ACC_TRAILER, eng.PVE_MAX_PARTS, eng.PVE_MAX_VERTS) == (vc.ROW, vc.TRAILER, vc.MAX_PARTS, 65536)
    for name, value in (('JRR_PVE_ACC_ROW', vc.ROW), ('JRR_PVE_ACC_HIST_PA', vc.HIST_PA), ('JRR_PVE_ACC_PART', vc.PART), ('JRR_PVE_ACC_PART_PA', vc.PART_PA),
                        ('JRR_PVE_ACC_LAYOUT_VERSION', 1)):
        assert f'{name} = {value},' in hdr, name
