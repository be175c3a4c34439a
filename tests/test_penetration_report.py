"""The self-penetration report on the host: closed forms of the restatement (tests/penetration_cases.py), the conditions the GPU tests'
inputs must satisfy (asserted in float64: at most 1 % of a case's points may be left out of the exact comparisons; the body cases leave
out none), the classification and the accumulator restatement on hand-made values, `derive` / `markdown` / `write` / `load` on a
hand-made table, the flag checks, and header / library / tables held equal."""
import importlib
import os
import re

import numpy as np
import pytest

import depth_cases as dc
import penetration_cases as pc
from conftest import PKG_NAME, ROOT

F32, F64 = np.float32, np.float64


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


# ---- the restatement ----
def test_winding_number_of_closed_meshes_is_an_integer_and_agrees_with_the_depth_restatement():
    for v, f in (dc.octahedron(), dc.cube(), dc.sphere(2)):
        pts = np.array([[0, 0, 0], [0.1, -0.05, 0.02], [2.0, 0.3, 0.1]])
        w, status = pc.winding(v, f, pts)
        assert status == 0 and np.abs(w - [1, 1, 0]).max() < 1e-12
        assert np.abs(w - dc.depth(v, f, pts)['wind']).max() < 1e-12           # another order of the same sum
        back, _ = pc.winding(v, f[:, ::-1], pts)
        assert np.abs(back + w).max() < 1e-12
    v, f = dc.cube()
    w, status = pc.winding(v, np.concatenate([f, [[0, 1, 8]], [[-1, 2, 3]]]), pts)
    assert status == 1 and np.abs(w - [1, 1, 0]).max() < 1e-12                 # a face out of range is skipped
    bad = v.copy()
    bad[3, 1] = np.nan
    assert np.isnan(pc.winding(bad, f, pts)[0]).all()
    pts[1, 2] = np.inf
    assert np.isnan(pc.winding(v, f, pts)[0]).tolist() == [False, True, False]


def test_classification_on_and_around_the_thresholds():
    w = np.array([0.0, 0.4, 0.5, 0.5000001, 0.89, 0.91, 1.0, -1.0, 1.09, 1.11, 1.5, 1.5000001, 1.9, -1.95, 2.1, 2.5, 3.0, np.nan], dtype=F32)
    k, pen, thin, uns = pc.classify(w)
    assert k[:-1].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 3]          # rintf rounds a half to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    assert pen.tolist() == [False] * 10 + [True] * 7 + [False]
    assert thin.tolist() == [True] * 3 + [False] * 15
    assert uns.tolist() == [False, True, True, True, True, False, False, False, False, True, True, True, True, False, False, True, False, False]      # 2 - 1.9f = 0.10000002 > 0.1f; 2.1f - 2 = 0.09999990
    assert [pc.n_bits(n) for n in (0, 1, 2, 3, 4, 7, 8, 300, 1 << 14, 1 << 20)] == [0, 1, 2, 2, 3, 3, 4, 9, 15, 21]


@pytest.mark.parametrize('name', pc.SMALL + ('body',))
def test_at_most_one_percent_of_a_case_is_left_out_of_the_exact_comparisons(name):
    ok = pc.check_cap(name)
    d = pc.distance(name)
    print(f'{name}: {int((~ok).sum())} of {ok.size} points left out; float32 restatement from float64 d {d:.2e}, bound {dc.bound(d):.2e}')
    k64 = pc.classify(pc.reference(name))[0]
    k32 = pc.classify(pc.reference(name, 'f32'))[0]
    assert np.array_equal(k64[ok], k32[ok]) and d < 1e-4
    if name == 'body':
        assert (~ok).sum() == 0


def test_sphere_cases_give_the_stated_integers():
    c, k = pc.small_case('two_spheres'), pc.classify(pc.reference('two_spheres'))[0][0]
    p, own = c['points'][0].astype(F64), c['part']
    other = np.linalg.norm(p - np.where(own[:, None] == 0, [1.0, 0, 0], [0.0, 0, 0]), axis=1)          # distance to the OTHER sphere's centre
    deep, clear = other < 0.9, other > 1.0          # the polyhedron's faces lie between radius 0.94 and 1
    assert deep.sum() >= 20 and clear.sum() >= 80 and (k[deep] == 2).all() and (k[clear] == 1).all() and set(k.tolist()) == {1.0, 2.0}
    back, _ = pc.winding(c['verts'][0], c['faces'][:, ::-1], c['points'][0])
    assert np.abs(back + pc.reference('two_spheres')[0]).max() < 1e-12
    c, k = pc.small_case('nested'), pc.classify(pc.reference('nested'))[0][0]
    assert (k[c['part'] == 1] == 2).all() and (k[c['part'] == 0] == 1).all() and (c['part'] == 1).sum() == 66
    assert pc.classify(pc.reference('three_spheres'))[0].max() == 3
    c = pc.small_case('octa_cube')
    assert c['faces'].shape == (20, 3) and c['faces'].shape[0] % 16 != 0
    assert set(pc.classify(pc.reference('octa_cube'))[0][0].tolist()) == {0.0, 1.0, 2.0}                # outside, inside one, inside both
    c = pc.small_case('row')
    assert c['verts'].shape == (1, 1290, 3) and c['faces'].shape == (2560, 3) and dc.is_closed(c['faces'])
    assert set(pc.classify(pc.reference('row'))[0][0].tolist()) == {1.0, 2.0}


def test_the_side_bend_penetrates_and_the_template_does_not():
    c, w = pc.body_case(), pc.reference('body')
    assert c['sign'] == -1 and dc.is_closed(c['faces'])          # the synthetic body is wound inwards: nothing may assume +1
    k, pen, thin, uns = pc.classify(w)
    print('template: pen', int(pen[0].sum()), 'thin', int(thin[0].sum()), ' bend: pen', int(pen[1].sum()), 'thin', int(thin[1].sum()), ' unsure',
          int(uns.sum()), ' parts of the bend', np.unique(c['part'][pen[1]]).tolist())
    assert pen[1].sum() >= 300 and pen[0].sum() <= 4 and uns[0].sum() == 0 and uns[1].sum() == 0
    assert np.array_equal(k[1], k[2])                            # the rigidly moved copy: the same integer at every vertex
    assert (np.sign(w[0][k[0] == 1]) == -1).all()


# ---- the accumulator restatement ----
def test_accumulate_restatement_on_hand_made_values():
    wind = np.ones((6, 40), dtype=F32)
    wind[0, :3] = [2.0, -2.1, 1.6]              # three penetrating, the last unsure too
    wind[0, 5:7] = [0.2, 0.45]                  # two thin, both unsure
    wind[1, :9] = 2.0                           # nine penetrating: also in POSES_PEN8
    wind[2, 4] = np.nan                         # bad
    wind[3, 0] = 3.0                            # group -1: counted nowhere but in its counts
    wind[4, 0] = 2.0                            # group 2 of 2: trailer word 1
    part = (np.arange(40) % 4).astype(np.int32)
    part[1], part[2] = -1, 40
    group = np.array([0, 1, 0, -1, 2, 1], dtype=np.int32)
    t, pv, counts = pc.accumulate(wind, part, group, 2)
    rows = t[:2 * pc.ROW].reshape(2, pc.ROW)
    assert counts.tolist() == [[3, 9, 0, 1, 1, 0], [2, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0]]
    assert rows[0, :7].tolist() == [1, 1, 1, 0, 3, 2, 3] and rows[1, :7].tolist() == [2, 0, 1, 1, 9, 0, 0]
    assert rows[0, pc.HIST:pc.HIST + 16].tolist() == [0, 0, 1] + [0] * 13 and rows[1, pc.HIST:pc.HIST + 16].tolist() == [1, 0, 0, 0, 1] + [0] * 11
    assert rows[0, pc.PART:pc.PART + 32].tolist() == [1] + [0] * 30 + [2]          # labels -1 and 40 go to word 31
    assert rows[1, pc.PART:pc.PART + 4].tolist() == [3, 1, 1, 2] and rows[1, pc.PART + 31] == 2
    assert t[-2:].tolist() == [1, 1] and pv[:9].tolist() == [2, 2, 2, 1, 1, 1, 1, 1, 1] and pv.sum() == 12
    t0, _, _ = pc.accumulate(wind, None, None, 1)
    assert t0[pc.COUNT] == 5 and t0[pc.BAD] == 1 and t0[pc.PART] == 3 + 9 + 1 + 1 and t0[pc.PART + 1:pc.PART + 32].sum() == 0


# ---- derive, markdown, the files ----
def _doc(tmp_path):
    pr = _mod('penetration_report')
    t, pv = pc.hand_made_table()
    part = np.zeros(6890, dtype=np.int32)
    part[:1000] = 3
    res = pr.derive(t, pv, ['Walking', 'Sitting'], part, 24)
    counts = np.zeros((3, 8), dtype=np.int32)
    counts[0] = [0, 300, 9, 1, 0, 9, 0, 0]
    counts[1] = 689
    res['counts'] = counts
    return pr, pr.write(str(tmp_path), res, ['Walking', 'Sitting'], 'action', 'vertices', 2.0, -1), res


def test_derive_on_a_hand_made_table(tmp_path):
    pr, doc, res = _doc(tmp_path)
    r = res['groups']['Walking']
    assert (r['n'], r['n_bad'], r['poses_pen'], r['poses_pen8']) == (4, 1, 3, 2)
    assert r['share_pen'] == 0.75 and r['share_pen8'] == 0.5 and r['mean_n_pen'] == 77.5
    assert r['share_thin'] == 0.1 and r['share_unsure'] == 2 / (4 * 6890)
    assert r['hist'] == [1, 1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert r['per_part']['Pelvis'] == 200 and r['per_part']['Spine1'] == 100 and sum(r['per_part'].values()) == 300          # word 31 is no part of 24
    e = res['groups']['Sitting']
    assert e['n'] == 0 and e['share_pen'] is None and e['mean_n_pen'] is None and e['share_thin'] is None
    assert res['all']['raw'] == r['raw'] and res['ignored'] == 3 and res['parts']['Spine1'] == 1000 and res['parts']['Pelvis'] == 5890
    bad = pc.hand_made_table()[0]
    bad[-1] = 2
    with pytest.raises(RuntimeError, match='group id'):
        pr.derive(bad, np.zeros(6890, dtype=np.int64), ['Walking', 'Sitting'])
    with pytest.raises(ValueError):
        pr.derive(bad[:-1], np.zeros(6890, dtype=np.int64), ['Walking', 'Sitting'])
    with pytest.raises(ValueError):
        pr.derive(bad.astype(np.int32), np.zeros(6890, dtype=np.int64), ['Walking', 'Sitting'])


def test_files_round_trip_and_markdown_rows(tmp_path):
    pr, doc, res = _doc(tmp_path)
    assert sorted(os.listdir(tmp_path)) == ['penetration.json', 'penetration.md', 'penetration.npz', 'penetration_per_vertex.npy']
    back = pr.load(str(tmp_path))
    import json
    assert back == json.loads(json.dumps(doc, sort_keys=True, default=str))
    assert back['worst'] == [{'index': 1, 'n_pen': 300, 'n_thin': 689, 'n_unsure': 0}, {'index': 2, 'n_pen': 9, 'n_thin': 689, 'n_unsure': 0},
                             {'index': 5, 'n_pen': 9, 'n_thin': 689, 'n_unsure': 0}, {'index': 3, 'n_pen': 1, 'n_thin': 689, 'n_unsure': 0}]
    pv = np.load(tmp_path / 'penetration_per_vertex.npy')
    assert pv.dtype == np.int64 and pv.shape == (6890,) and np.array_equal(pv, pc.hand_made_table()[1])
    assert back['per_vertex'] == {'file': 'penetration_per_vertex.npy', 'n_ever': 11, 'max': 4, 'argmax': 100}
    z = np.load(tmp_path / 'penetration.npz')
    assert sorted(z.files) == ['n_pen', 'n_thin', 'n_unsure'] and all(z[k].dtype == np.int32 and z[k].shape == (8,) for k in z.files)
    assert z['n_pen'].tolist() == [0, 300, 9, 1, 0, 9, 0, 0]
    md = open(tmp_path / 'penetration.md').read()
    assert '| Walking | 4 | 1 | 3 | 75.00 | 2 | 50.00 | 77.50 | 10.00 | 0.01 |' in md
    assert '| Sitting | 0 | 0 | 0 | - | 0 | - | - | - | - |' in md and '| all | 4 | 1 | 3 | 75.00 |' in md
    assert '| n_pen | 0 | 1 | 2-3 | 4-7 | 8-15 |' in md and '| poses | 1 | 1 | 0 | 0 | 1 | 0 | 0 | 0 | 0 | 1 |' in md
    assert '| Spine1 | 1000 | 100 | 25.00 |' in md and '| 1 | 300 | 689 | 0 |' in md and 'winding -1 inside' in md and '2 mm' in md
    assert '3 samples were not scored' in md
    assert 'self-penetration (2 mm push): 75.00 % of the poses penetrate, 50.00 % with 8' in pr.summary_line(doc)
    doc['layout_version'] = 0
    with open(tmp_path / 'penetration.json', 'w') as f:
        json.dump(doc, f, default=str)
    with pytest.raises(ValueError, match='layout version'):
        pr.load(str(tmp_path))


def test_orientation_is_the_sign_of_the_signed_volume():
    pr = _mod('penetration_report')
    v, f = dc.cube()
    nan = np.full_like(v, np.nan)
    assert pr.orientation(np.stack([nan, v]), f) == 1 and pr.orientation(v[None], f[:, ::-1]) == -1          # the first FINITE mesh
    assert pr.orientation(pc.body_case()['verts'], pc.body_case()['faces']) == -1
    with pytest.raises(ValueError, match='volume of zero'):
        pr.orientation(np.zeros((1, 8, 3)), f)
    with pytest.raises(ValueError, match='no mesh'):
        pr.orientation(nan[None], f)


# ---- flags ----
def test_flag_errors(tmp_path):
    pr, argsmod = _mod('penetration_report'), _mod('args')
    ok = ['--eval_vertices', str(tmp_path), '--eval_report', str(tmp_path / 'out'), '--synthetic', '--smpl_dir', '/nonexistent']
    pr.check_flags(argsmod.get_args(ok))                                                          # the flag is off
    pr.check_flags(argsmod.get_args(ok + ['--eval_penetration']))
    pr.check_flags(argsmod.get_args(ok + ['--eval_penetration', '--eval_penetration_offset_mm', '10']))
    assert argsmod.get_args(ok).eval_penetration_offset_mm == 2.0
    for flags, what in ((['--eval_report', 'x', '--synthetic', '--eval_penetration'], 'needs --eval_vertices'),
                        (['--eval_vertices', 'x', '--synthetic', '--eval_penetration'], 'needs --eval_vertices'),
                        (ok[:4] + ['--smpl_dir', '/nonexistent', '--eval_penetration'], 'body model'),
                        (ok + ['--eval_penetration', '--eval_penetration_offset_mm', '0'], 'offset_mm'),
                        (ok + ['--eval_penetration', '--eval_penetration_offset_mm', '-1'], 'offset_mm'),
                        (ok + ['--eval_penetration', '--eval_penetration_offset_mm', '10.5'], 'offset_mm'),
                        (ok + ['--eval_penetration', '--eval_penetration_offset_mm', 'nan'], 'offset_mm'),
                        (ok + ['--eval_penetration', '--eval_penetration_offset_mm', 'inf'], 'offset_mm')):
        with pytest.raises(ValueError, match=what):
            pr.check_flags(argsmod.get_args(flags))
    ns = argsmod.get_args(ok + ['--eval_penetration'])
    assert 'eval_penetration' not in pr.flags_doc(ns) and 'eval_penetration_offset_mm' not in pr.flags_doc(vars(ns)) and 'eval_report' in pr.flags_doc(ns)


def test_the_driver_refuses_before_any_launch(tmp_path):
    argsmod, er = _mod('args'), _mod('eval_report')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(['--eval_vertices', str(tmp_path), '--eval_report', str(tmp_path / 'out'), '--smpl_dir', '/nonexistent',
                                              '--eval_penetration'])
    try:
        with pytest.raises(ValueError, match='body model'):
            er.evaluate_vertices(log=lambda s: None)
    finally:
        argsmod._LazyArgs._ns = saved
    assert not (tmp_path / 'out').exists()
    # the parameter path scores no directory of meshes: the flag is refused there, before any launch
    argsmod._LazyArgs._ns = argsmod.get_args(['--synthetic', '--eval_report', str(tmp_path / 'out'), '--eval_penetration'])
    try:
        with pytest.raises(ValueError, match='needs --eval_vertices'):
            _mod('test').test_pose_refiner_model(log=lambda s: None)
    finally:
        argsmod._LazyArgs._ns = saved
    assert not (tmp_path / 'out').exists()


# ---- header, library and tables held equal ----
def test_header_library_and_python_tables_agree():
    text = open(os.path.join(ROOT, 'include', 'jrr.h')).read()
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r'\b(JRR_(?:PEN_ACC|WINDING)_\w+) = (\d+)', text)}
    pr, eng = _mod('penetration_report'), _mod('engine')
    for mod in (pc, pr):
        assert (mod.ROW, mod.TRAILER, mod.BINS, mod.COUNT, mod.BAD, mod.POSES_PEN, mod.POSES_PEN8, mod.SUM_PEN, mod.SUM_THIN, mod.SUM_UNSURE, mod.HIST,
                mod.PART) == tuple(enum['JRR_PEN_ACC_' + k] for k in ('ROW', 'TRAILER', 'BINS', 'COUNT', 'BAD', 'POSES_PEN', 'POSES_PEN8', 'SUM_PEN',
                                                                        'SUM_THIN', 'SUM_UNSURE', 'HIST', 'PART'))
    assert pr.LAYOUT_VERSION == enum['JRR_PEN_ACC_LAYOUT_VERSION'] and pr.MAX_PARTS == pc.PARTS == enum['JRR_PEN_ACC_PARTS']
    assert enum['JRR_PEN_ACC_ROW'] == enum['JRR_PEN_ACC_PART'] + enum['JRR_PEN_ACC_PARTS'] and enum['JRR_PEN_ACC_PART'] == enum['JRR_PEN_ACC_HIST'] + enum['JRR_PEN_ACC_BINS']
    assert (eng.PEN_ACC_ROW, eng.PEN_ACC_TRAILER, eng.WINDING_MAX_POINTS) == (enum['JRR_PEN_ACC_ROW'], enum['JRR_PEN_ACC_TRAILER'], enum['JRR_WINDING_MAX_POINTS'])
    assert pc.MAX_POINTS == enum['JRR_WINDING_MAX_POINTS'] and len(pr.HIST_LABELS) == pr.BINS
    assert 'f mod 4' in text and '(s0 + s1) + (s2 + s3)' in text          # the order of the sum is written in the header
    table = _mod('_lib')
    src = open(table.__file__).read()
    assert "'jrr_mesh_winding'" in src and "'jrr_penetration_accumulate'" in src
    assert 'pen.hip' in _mod('build').SOURCES and os.path.isfile(os.path.join(os.path.dirname(table.__file__), 'csrc', 'pen.hip'))
    for name in ('jrr_mesh_winding', 'jrr_penetration_accumulate'):
        assert re.search(r'\bint ' + name + r'\(', text)
