"""The depth section of the regressor report on the host: closed forms of the restatement (tests/depth_cases.py), the conditions the
GPU tests' inputs must satisfy (asserted in float64: a seed that breaks one is replaced, the condition never relaxed), the accumulator
restatement and `derive_depth` on a hand-made table, the flag checks, and header / library / tables held equal."""
import importlib
import os
import re

import numpy as np
import pytest

import depth_cases as dc
from conftest import PKG_NAME, ROOT

F32, F64 = np.float32, np.float64


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


# ---- closed forms ----
def test_octahedron_and_cube_centres():
    v, f = dc.octahedron()
    r = dc.depth(v, f, np.zeros((1, 3)))
    assert abs(r['dist'][0] - 1 / np.sqrt(3)) < 1e-15 and abs(abs(r['wind'][0]) - 1) < 1e-15 and r['region'][0] == 6
    v, f = dc.cube()
    r = dc.depth(v, f, np.zeros((1, 3)))
    assert abs(r['dist'][0] - 0.5) < 1e-15 and abs(abs(r['wind'][0]) - 1) < 1e-15
    assert dc.is_closed(dc.octahedron()[1]) and dc.is_closed(dc.cube()[1])
    assert not dc.is_closed(dc.cube()[1][:-1])


def test_points_over_a_face_beyond_an_edge_and_beyond_a_corner_of_the_cube():
    v, f = dc.cube()
    h = 0.25
    pts = np.array([[0.1, -0.2, 0.5 + h],            # over the face z = +0.5
                    [0.1, -0.2, 0.5 - h],            # under it, inside
                    [0.5 + h, 0.5 + h, 0.1],         # beyond the edge x = y = 0.5
                    [0.5 + h, 0.5 + h, 0.5 + h],     # beyond the corner
                    [0.5, 0.5, 0.5 + h]])            # straight above the corner
    r = dc.depth(v, dc._relabel(f), pts)
    want = [h, h, h * np.sqrt(2), h * np.sqrt(3), h]
    assert np.abs(r['dist'] - want).max() < 1e-15
    assert np.abs(r['wind'] - [0, 1, 0, 0, 0]).max() < 1e-15
    assert r['region'][0] == 6 and r['region'][1] == 6 and dc.REGIONS[r['region'][2]] in ('ab', 'ac', 'bc') and dc.REGIONS[r['region'][3]] in ('a', 'b', 'c')
    # the corner is shared: every face that holds it computes the same distance, and the smallest index is reported
    corner = 7
    holders = np.flatnonzero((f == corner).any(axis=1))
    assert holders.size >= 3 and np.all(r['all'][4, holders] == h) and r['face'][4] == holders.min()


def test_sphere_meshes_have_the_stated_sizes_and_are_closed():
    for levels, (nv, nf) in ((2, (66, 128)), (3, (258, 512))):
        v, f = dc.sphere(levels)
        assert v.shape == (nv, 3) and f.shape == (nf, 3) and dc.is_closed(f) and np.abs(np.linalg.norm(v, axis=1) - 1).max() < 1e-12
        r = dc.depth(v, f, np.array([[0, 0, 0], [2.0, 0.3, 0.1]]))
        assert np.abs(r['wind'] - [1, 0]).max() < 1e-12


def test_defective_faces_in_the_restatement():
    v, f = dc.cube()
    pts = np.array([[0.1, 0.2, 0.3], [0.9, 0.1, 0.0]])
    base = dc.depth(v, f, pts)
    flat = dc.depth(v, np.concatenate([f, [[3, 3, 5]]]), pts)               # a zero-area face: NaN, never the minimum
    assert np.isnan(flat['all'][:, -1]).all() and np.array_equal(flat['dist'], base['dist']) and np.array_equal(flat['face'], base['face'])
    assert np.abs(flat['wind'] - base['wind']).max() < 1e-15
    out = dc.depth(v, np.concatenate([[[0, 1, 8]], f]), pts)                # an index out of range: skipped, status bit 0
    assert out['status'] == 1 and base['status'] == 0 and np.array_equal(out['dist'], base['dist']) and np.array_equal(out['face'], base['face'] + 1)
    back = dc.depth(v, f[:, ::-1], pts)                                     # re-wound
    assert np.abs(back['wind'] + base['wind']).max() < 1e-15 and np.abs(back['dist'] - base['dist']).max() < 1e-15


# ---- the conditions on the GPU tests' inputs ----
def test_gpu_inputs_cover_all_seven_regions_and_keep_clear_of_the_surface():
    seen = np.zeros(7, dtype=np.int64)
    for name in dc.CONVEX + ('body',):
        v, f, p = dc.case(name)
        r = dc.reference(name)
        assert dc.is_closed(f) and r['status'] == 0, name
        seen += np.bincount(r['region'].ravel(), minlength=7)
        dc.check_inside_conditions(r)                                       # the inside flag is not a matter of rounding
        d = np.abs(dc.reference(name, 'f32')['dist'].astype(F64) - r['dist']).max()
        w = np.abs(dc.reference(name, 'f32')['wind'].astype(F64) - r['wind']).max()
        print(f'{name}: float32 restatement against float64: dist {d:.2e} m (bound {dc.bound(d):.2e}), wind {w:.2e} (bound {dc.bound(w):.2e})')
        assert d < 1e-6 and w < 1e-5, name
    print('regions of the nearest faces:', dict(zip(dc.REGIONS, seen.tolist())))
    assert (seen > 0).all(), dict(zip(dc.REGIONS, seen.tolist()))


def test_driver_inputs_keep_clear_of_the_surface_and_push_one_joint_through_the_skin():
    c = dc.driver_case()
    r = dc.depth_batch(c['verts'], c['faces'], dc.driver_points_host())
    print(f'driver inputs: nearest point {r["dist"].min() * 1000:.2f} mm from the surface')
    dc.check_inside_conditions(r)
    assert r['dist'].shape == (6, 51) and r['status'] == 0
    outside = np.abs(r['wind']) < 0.5
    assert not outside[:, :17].any() and not outside[:, 34:].any()         # the initial regressor and the ground truth: all inside
    assert outside[:, 17:34].sum(0).tolist() == [0] * 16 + [6]               # the retrained R_Wrist: outside in every pose
    assert (r['dist'][:, 33] > 5e-3).all()


def test_the_body_is_closed_wound_inwards_and_holds_the_shipped_joints():
    v, f, p = dc.body_case()
    assert v.shape == (3, 6890, 3) and f.shape == (13776, 3) and dc.is_closed(f)
    r = dc.reference('body')
    assert np.abs(r['wind'][:, :17] + 1).max() < 1e-9                       # -1 inside: nothing may assume +1
    moved = r['wind'][:, 17:]                                               # shifted by half a metre: outside, or inside another limb
    assert np.minimum(np.abs(moved), np.abs(moved + 1)).max() < 1e-9 and (np.abs(moved) < 1e-9).mean() > 0.9
    template = r['dist'][0, :17]
    print(f'shipped joints on the template: nearest {template.min() * 1000:.2f} mm below the skin (joint {template.argmin()})')
    assert abs(template.min() * 1000 - 1.45) < 0.01


# ---- the accumulator and derive ----
def test_accumulator_restatement_on_known_values():
    dist = np.array([[0.010, 0.002, 0.5], [0.010, 0.002, 0.5], [np.nan, 0.1, 0.1], [0.01, 0.01, 1.0e3], [0.3, 0.2, 0.1]], dtype=F32)
    wind = np.array([[-1, 0, 0.3], [1, 1, 2], [1, 1, 1], [1, 1, 1], [1, 1, 1]], dtype=F32)
    group = np.array([0, 1, 0, 1, -1], dtype=np.int32)
    t = dc.accumulate(dist, wind, group, 2)
    t = dc.accumulate(dist[:1], wind[:1], np.array([2], dtype=np.int32), 2, t)
    r0, r1 = t[:dc.ROW], t[dc.ROW:2 * dc.ROW]
    assert (r0[dc.COUNT], r0[dc.BAD], r1[dc.COUNT], r1[dc.BAD]) == (1, 1, 1, 1) and t[2 * dc.ROW:].tolist() == [1, 1]
    assert r0[dc.OUTSIDE:dc.OUTSIDE + 3].tolist() == [0, 1, 1] and r0[dc.UNSURE:dc.UNSURE + 3].tolist() == [0, 0, 1]
    assert r1[dc.OUTSIDE:dc.OUTSIDE + 3].tolist() == [0, 0, 0] and r1[dc.UNSURE:dc.UNSURE + 3].tolist() == [0, 0, 0]
    q = lambda x: int(np.rint(F64(F32(x) * F32(16777216.0))))
    assert r0[dc.SUM:dc.SUM + 3].tolist() == [q(0.010), -q(0.002), -q(0.5)]
    hist = r0[dc.HIST:].reshape(64, 64)
    assert hist[0, 18] == 1 and hist[1, 15] == 1 and hist[2, 0] == 1 and hist.sum() == 3      # [8, 12), [-4, 0), clamped below
    assert r1[dc.HIST:].reshape(64, 64)[2, 63] == 1                                             # 500 mm: clamped above
    assert t[dc.HIST + 3 * 64:dc.ROW].sum() == 0                                                # columns >= n_points untouched


def test_derive_depth_on_a_hand_made_table():
    rr = _mod('regressor_report')
    doc = rr.derive_depth(dc.hand_made_table(), ['Walking', 'Sitting'])
    g, empty = doc['groups']['Walking'], doc['groups']['Sitting']
    assert (g['n'], g['n_bad'], empty['n'], doc['ignored']) == (4, 1, 0, 3) and doc['all']['n'] == 4
    assert all(empty['sets'][s][k] is None for s in rr.DEPTH_SETS for k in rr.DEPTH_KEYS)
    ini, ret, gt = (g['sets'][s] for s in rr.DEPTH_SETS)
    assert abs(ini['mean_mm'][0] - 10.0) < 1e-4 and abs(ret['mean_mm'][3] + 2.0) < 1e-4 and ini['mean_mm'][1] == 0.0
    assert ret['outside'][3] == 0.25 and sum(ret['outside']) == 0.25 and sum(ini['outside']) == 0 and gt['unsure'][5] == 0.5
    assert ini['median_mm'][0] == 12.0 and ini['p05_mm'][0] == 12.0           # upper edges of [8, 12)
    assert ret['median_mm'][3] == 12.0 and ret['p05_mm'][3] == 0.0            # one of four in [-4, 0)
    assert rr.newly_outside(doc) == [3]
    bad = dc.hand_made_table()
    bad[2 * dc.ROW + 1] = 2
    with pytest.raises(RuntimeError, match='group id'):
        rr.derive_depth(bad, ['Walking', 'Sitting'])
    with pytest.raises(ValueError):
        rr.derive_depth(bad[:-1], ['Walking', 'Sitting'])
    # the markdown flags the joint
    tpl = {'orientation': -1, 'initial': {'depth_mm': [5.0] * 17}, 'retrained': {'depth_mm': [4.0] * 17}}
    md = rr.depth_markdown({'source': 'vertices', 'groups': ['Walking', 'Sitting'], 'data': doc, 'template': tpl, 'newly_outside': rr.newly_outside(doc)})
    name = _mod('eval_report').JOINT_NAMES[3]
    assert f'{name} **!**' in md and 'winding -1 inside' in md and md.count('**!**') == 1


# ---- flags, header, library ----
def test_flag_checks_and_their_messages():
    a, rr = _mod('args'), _mod('regressor_report')
    assert a.get_args([]).regressor_report_depth is False
    with pytest.raises(ValueError, match='--regressor_report DIR'):
        rr.check_flags(a.get_args(['--regressor_report_depth', '--synthetic']))
    with pytest.raises(ValueError, match='faces of the body model'):
        rr.check_flags(a.get_args(['--regressor_report_depth', '--regressor_report', 'out', '--smpl_dir', '/nonexistent']))
    rr.check_flags(a.get_args(['--regressor_report_depth', '--regressor_report', 'out', '--smpl_dir', '/nonexistent', '--synthetic']))
    assert rr.body_model_available('/nonexistent', False) is False and rr.body_model_available(None, True) is True
    # a driver that holds a body model of its own needs none resolved
    rr.check_flags(a.get_args(['--regressor_report_depth', '--regressor_report', 'out', '--smpl_dir', '/nonexistent']), have_model=True)
    # the parameter path refuses the flag without the report too, before anything is loaded or launched (this test has no GPU)
    argsmod, saved = a, a._LazyArgs._ns
    argsmod._LazyArgs._ns = a.get_args(['--regressor_report_depth', '--synthetic'])
    try:
        with pytest.raises(ValueError, match='--regressor_report DIR'):
            _mod('test').test_pose_refiner_model(log=lambda s: None)
    finally:
        argsmod._LazyArgs._ns = saved
    # the flag changes none of the existing files, so none records it
    on = rr.flags_doc(a.get_args(['--regressor_report_depth']))
    assert 'regressor_report_depth' not in on and on == rr.flags_doc(vars(a.get_args([])))


def test_header_library_and_tables_agree():
    hdr = open(os.path.join(ROOT, 'include', 'jrr.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    val = lambda name: int(re.search(r'\b%s\s*=\s*(\d+)' % name, hdr).group(1))
    rr, eng, lib_mod, b = _mod('regressor_report'), _mod('engine'), _mod('_lib'), _mod('build')
    assert (dc.ROW, dc.COUNT, dc.BAD, dc.OUTSIDE, dc.UNSURE, dc.SUM, dc.HIST, dc.BINS, dc.TRAILER) == tuple(
        val('JRR_DEPTH_ACC_' + k) for k in ('ROW', 'COUNT', 'BAD', 'OUTSIDE', 'UNSURE', 'SUM', 'HIST', 'BINS', 'TRAILER'))
    assert (rr.D_ROW, rr.D_OUTSIDE, rr.D_UNSURE, rr.D_SUM, rr.D_HIST, rr.D_BINS) == (dc.ROW, dc.OUTSIDE, dc.UNSURE, dc.SUM, dc.HIST, dc.BINS)
    assert rr.DEPTH_LAYOUT_VERSION == val('JRR_DEPTH_ACC_LAYOUT_VERSION') and dc.ROW == dc.HIST + 64 * dc.BINS
    assert (eng.DEPTH_MAX_POINTS, eng.DEPTH_MAX_VERTS, eng.DEPTH_ACC_ROW, eng.DEPTH_ACC_TRAILER, eng.DEPTH_STATUS_INDEX) == (
        val('JRR_DEPTH_MAX_POINTS'), val('JRR_DEPTH_MAX_VERTS'), dc.ROW, dc.TRAILER, val('JRR_DEPTH_STATUS_INDEX'))
    b.build(verbose=False)
    lib = lib_mod.load()
    for name, n_args in (('jrr_point_mesh_depth', 12), ('jrr_depth_accumulate', 8)):
        assert re.search(r'\b%s\s*\(' % name, hdr) and hasattr(lib, name) and f'`{name}`' in doc, name
        assert len(lib_mod.SIGNATURES[name][1]) == n_args
    assert 'depth.hip' in b.SOURCES


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes
    lib_mod = _mod('_lib')
    _mod('build').build(verbose=False)
    lib = lib_mod.load()
    P = ctypes.c_void_p
    ok = P(4096)                                   # never dereferenced: every call below is refused on the host
    call = lambda **kw: lib.jrr_point_mesh_depth(*[kw.get(k, d) for k, d in (
        ('verts', ok), ('batch', 1), ('n_verts', 8), ('faces', ok), ('n_faces', 12), ('points', ok), ('n_points', 17), ('dist', ok), ('wind', ok),
        ('face', ok), ('status', ok), ('stream', None))])
    for kw, word in (({'verts': None}, 'NULL'), ({'status': None}, 'NULL'), ({'dist': None, 'wind': None, 'face': None}, 'all NULL'),
                     ({'n_points': 0}, 'points'), ({'n_points': 65}, '1 .. 64 points'), ({'n_verts': 8193}, '8192'), ({'n_faces': 0}, 'faces'),
                     ({'batch': -1}, 'batch'), ({'verts': P(4100)}, 'misaligned'), ({'points': P(4098)}, 'misaligned')):
        assert call(**kw) == -1 and word.encode() in lib.jrr_last_error(), (kw, lib.jrr_last_error())
    assert call(batch=0) == 0
    acc = lambda **kw: lib.jrr_depth_accumulate(*[kw.get(k, d) for k, d in (
        ('dist', ok), ('wind', ok), ('group', None), ('batch', 1), ('n_points', 51), ('n_groups', 3), ('acc', ok), ('stream', None))])
    for kw in ({'dist': None}, {'acc': None}, {'acc': P(4100)}, {'n_points': 65}, {'n_groups': 0}, {'n_groups': 1025}, {'batch': -1}):
        assert acc(**kw) == -1 and b'jrr_depth_accumulate' in lib.jrr_last_error(), kw
    assert acc(batch=0) == 0
