"""The view fusion over the refined-pose table without a GPU: the groups of views (refined.view_key, refined.view_groups), the 4x4 solves
(refined.relative_rotations), the float64 restatement (tests/view_fuse_cases.py) with its case builders' own assertions, the C ABI rows,
the refined_fused.npz / meta.json files through refined.fuse_views with the three operators replaced by the host restatement, and the
flags."""
import importlib
import json
import os
import pickle
import re

import numpy as np
import pytest
import torch

import refined_cases as rc
import view_fuse_cases as vc
from conftest import PKG_NAME, ROOT

F = np.float32
T = torch.from_numpy


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _path(action, camera, frame, subject='S9'):
    return f'/data/h36m/{subject}/{action}/imageSequence/{camera}/img_{frame:06d}.jpg'


# ---- 1. groups of views ----
def test_view_key():
    refined = _mod('refined')
    assert refined.view_key(_path('Walking 1', '55011271', 12)) == ('/data/h36m/S9/Walking 1', '55011271', 12)
    assert refined.view_key('S9\\Eating\\imageSequence\\c2\\img_000310.png') == ('S9/Eating', 'c2', 310)
    for bad in ('/data/frames/000012.jpg', '/data/S9/Eating/imageSequence/img_000001.jpg', '/data/S9/Eating/imageSequence/5/frame12.jpg', '', None):
        assert refined.view_key(bad) == (None, None, -1), bad
        assert refined.sequence_key(bad) == (None, -1)


def _rig_paths():
    """two scenes in a non-monotone file order: `Walking` with cameras 1 - 4 over frames 1 - 5 (camera 3 misses frames 2 and 4, frame 3 of
    camera 2 is there twice, frame 5 of camera 4 is unrefined), `Eating` with cameras 2 and 4 over frames 7 and 8, one stray path"""
    rows = [('Walking', c, f) for f in (3, 1, 5, 2, 4) for c in ('4', '2', '1', '3') if not (c == '3' and f in (2, 4))]
    rows.insert(5, ('Walking', '2', 3))
    rows += [('Eating', c, f) for f in (8, 7) for c in ('4', '2')]
    paths = [_path(*r) for r in rows]
    paths.insert(9, '/data/elsewhere/000001.jpg')
    has = np.ones(len(paths), np.uint8)
    has[paths.index(_path('Walking', '4', 5))] = 0
    return paths, has


def test_view_groups_on_paths():
    refined = _mod('refined')
    paths, has = _rig_paths()
    order, group, pair, ref_pair, names, duplicates = refined.view_groups(paths, has)
    for a in (order, group, pair, ref_pair):
        assert a.dtype == np.int32 and a.ndim == 1
    assert names == [('/data/h36m/S9/Eating', '2'), ('/data/h36m/S9/Eating', '4')] + [('/data/h36m/S9/Walking', c) for c in '1234']
    assert ref_pair.tolist() == [0, 0, 2, 2, 2, 2] and duplicates == 1
    listed = [paths[i] for i in order]
    want = [_path('Eating', c, f) for f in (7, 8) for c in '24']
    want += [_path('Walking', c, 1) for c in '1234'] + [_path('Walking', c, 2) for c in '124']
    want += [_path('Walking', c, 3) for c in '1234'] + [_path('Walking', '2', 3)]
    want += [_path('Walking', c, 4) for c in '124'] + [_path('Walking', c, 5) for c in '123'] + ['/data/elsewhere/000001.jpg']
    assert listed == want
    assert group.tolist() == [0, 0, 1, 1] + [2] * 4 + [3] * 3 + [4] * 4 + [5] + [6] * 3 + [7] * 3 + [8]
    assert pair.tolist() == [0, 1, 0, 1] + [2, 3, 4, 5] + [2, 3, 5] + [2, 3, 4, 5] + [-1] + [2, 3, 5] + [2, 3, 4] + [-1]
    assert (np.diff(group) >= 0).all() and sorted(order.tolist()) == np.nonzero(has)[0].tolist() and (np.diff(order) < 0).any()
    dup_rows = [i for i, p in enumerate(paths) if p == _path('Walking', '2', 3)]
    assert order[group == 5].tolist() == [dup_rows[1]] and dup_rows[0] in order[group == 4]      # the later row is the duplicate
    # the restatement, by dictionaries, gives the same lists
    keys = [refined.view_key(p) for p in paths]
    mine = vc.view_groups([k[0] for k in keys], [k[1] for k in keys], [k[2] for k in keys], has)
    for a, b in zip(mine[:4], (order, group, pair, ref_pair)):
        assert np.array_equal(a, b)
    assert mine[4] == names and mine[5] == 1
    # nothing refined, and a wrong number of paths
    o, g, p, r, n, d = refined.view_groups(paths, np.zeros(len(paths)))
    assert o.shape == g.shape == p.shape == r.shape == (0,) and o.dtype == np.int32 and n == [] and d == 0
    with pytest.raises(ValueError, match='3 paths for a table of 4 rows'):
        refined.view_groups(['a', 'b', 'c'], np.ones(4))


def test_nine_cameras_in_one_frame_raise():
    refined = _mod('refined')
    paths = [_path('Posing', str(c), f) for f in (1, 2) for c in range(1, 9)]
    order, group, pair, ref_pair, names, _ = refined.view_groups(paths, np.ones(16))
    assert np.bincount(group).tolist() == [8, 8] and len(names) == 8
    with pytest.raises(ValueError, match='9 views of frame 2'):
        refined.view_groups(paths + [_path('Posing', '9', 2)], np.ones(17))
    # nine cameras of a scene, never more than eight at once, are fine; and a ninth row that is a duplicate does not count
    ok = refined.view_groups(paths[:15] + [_path('Posing', '9', 2), _path('Posing', '3', 1)], np.ones(17))
    assert np.bincount(ok[1]).tolist() == [8, 1, 8] and len(ok[4]) == 9 and ok[5] == 1


def test_arrays_in_place_of_paths():
    refined = _mod('refined')
    rng = np.random.RandomState(0)
    scenes, cams, frames = rng.randint(0, 2, size=80), rng.randint(0, 4, size=80), rng.randint(0, 12, size=80)
    frames[[7, 33]] = -1
    has = (rng.uniform(size=80) < 0.8).astype(np.uint8)
    paths = [_path(f'A{s}', str(c), f) if f >= 0 else '/nowhere/x.jpg' for s, c, f in zip(scenes, cams, frames)]
    by_path, by_arrays = refined.view_groups(paths, has), refined.view_groups((scenes, cams, frames), has)
    mine = vc.view_groups(scenes.tolist(), cams.tolist(), frames.tolist(), has)
    for a, b, c in zip(by_path[:4], by_arrays[:4], mine[:4]):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert by_path[5] == by_arrays[5] == mine[5] > 0 and by_arrays[4] == mine[4]
    order, group, pair = by_arrays[:3]
    same = group[1:] == group[:-1]
    assert same.any() and (np.diff(cams[order])[same] > 0).all() and (pair[np.isin(order, [7, 33])] == -1).all()
    # (cameras, frames): one scene
    one = refined.view_groups((cams, frames), has)
    assert np.array_equal(one[0], vc.view_groups([0] * 80, cams.tolist(), frames.tolist(), has)[0]) and len(one[4]) == 4
    # the lists of the GPU tests' table, from its own pair and group as camera and frame
    g, p, r = vc.group_lists()
    got = refined.view_groups((p, g), np.ones(vc.M))
    assert np.array_equal(got[0], np.arange(vc.M)) and np.array_equal(got[1], g) and np.array_equal(got[2], p) and np.array_equal(got[3], r)


# ---- 2. the 4 x 4 solves ----
def _acc_of(quaternions):
    acc = np.zeros(vc.ACC_ROW, np.int64)
    iu = np.triu_indices(4)
    for e in np.asarray(quaternions, dtype=F):
        acc[0] += 1
        acc[1:11] += np.rint((e[:, None] * e[None, :])[iu].astype(np.float64) * vc.FIX).astype(np.int64)
    return acc


def test_relative_rotations_on_a_hand_made_table():
    refined = _mod('refined')
    rng = np.random.RandomState(1)
    d = np.array([np.cos(0.4), 0.6 * np.sin(0.4), 0.0, -0.8 * np.sin(0.4)])                  # 0.8 rad about (0.6, 0, -0.8)
    noisy = vc.qmul(d[None], vc.quats(vc.sc.to_6d(vc.sc.expmap(rng.normal(scale=0.05, size=(400, 3))))))
    noisy *= rng.choice([-1.0, 1.0], size=(400, 1))                                         # the sign of a sample is immaterial
    acc = np.stack([_acc_of([[1, 0, 0, 0]] * 3), np.zeros(vc.ACC_ROW, np.int64), _acc_of(noisy), _acc_of([-d] * 5), np.zeros(vc.ACC_ROW, np.int64)])
    rel, res = refined.relative_rotations(acc, np.array([4, 4, 4, 4, 4]))
    assert rel.dtype == F and rel.shape == (5, 4) and res.shape == (5,)
    assert np.abs(rel[0] - [1, 0, 0, 0]).max() < 1e-6 and res[0] < 0.1                      # acos near 1: 1e-7 in lambda is 0.04 degrees
    assert not rel[1].any() and np.isnan(res[1])                                            # nobody counted: unknown
    angle = lambda a, b: np.degrees(2 * np.arccos(min(1.0, abs(float(np.dot(a, b))))))
    assert angle(rel[2], d) < 3 * 0.05 * np.sqrt(3.0 / 400) * 57.3 + 0.05 and rel[2][0] > 0
    assert 0.5 * np.degrees(0.05) < res[2] < 3 * np.degrees(0.05)                           # the spread: of the order of the noise
    assert np.abs(rel[3] - d).max() < 1e-6 and res[3] < 0.1                                 # w >= 0 whatever the samples' sign
    assert rel[4].tolist() == [1, 0, 0, 0] and res[4] == 0                                  # the reference camera itself
    mine = vc.solve(*vc.acc_mean(acc), np.array([4, 4, 4, 4, 4]))
    assert np.abs(mine[0] - rel).max() < 1e-6 and np.allclose(mine[1], res, atol=1e-3, equal_nan=True)
    assert refined.relative_rotations(acc)[0][4].tolist() == [0, 0, 0, 0]                    # without ref_pair nobody is a reference


# ---- 3. the restatement and its cases ----
def test_table_case_has_the_shapes_the_gpu_tests_rely_on():
    c = vc.table_case()
    x6d, betas = vc.positions_of(c['table'], c['order'])
    g, p = c['group'], c['pair']
    assert vc.M == 70 and g[31] == g[32] and g[63] == g[64] and np.bincount(g)[[g[32], g[64]]].tolist() == [8, 8]
    assert np.bincount(g).tolist() == list(vc.GROUP_SIZES) and (c['table'][:, 229] == 0).sum() == 26
    q = vc.quats(x6d)
    pairs = [(a, b) for a in range(vc.M) for b in range(a + 1, min(vc.M, a + 8)) if g[a] == g[b]]
    neg = np.array([(vc.qdot(q[a], q[b]) < 0) for a, b in pairs])
    assert neg[:, 3::4].any() and neg[:, 1::4].any()                                        # views whose quaternions have opposite signs
    ang = np.degrees(np.arccos(np.clip((np.trace(vc.rot6d(x6d[:, 1::4]), axis1=-2, axis2=-1) - 1) / 2, -1, 1)))
    assert (np.pi - np.radians(ang) < 0.05).mean() > 0.98                                   # within 1e-3 of pi, then perturbed; but for the outliers
    assert np.array_equal(x6d[:, 2::4], np.broadcast_to(F([1, 0, 0, 1, 0, 0]), (vc.M, 6, 6)))
    count, mean = vc.accumulate(x6d, g, p, c['ref_pair'])
    assert count[0] == 0 and count[8] == 0 and (count[1:8] > 0).all()                       # camera 8 never meets the reference camera
    for max_deg in (0.0, 30.0):
        r64, d, r32 = vc.yardstick(x6d, betas, g, p, c['rel'], max_deg)                     # asserts the branch conditions
        print(f'max_deg {max_deg:g}: float32 from float64: rotation {d[0]:.3e} betas {d[1]:.3e} body {d[2]:.3e} rad orient {d[3]:.3e} rad')
        assert max(d) <= 5e-6 and min(d[0], d[2]) > 0
        assert r64['members'].tolist() == np.repeat(vc.GROUP_SIZES, vc.GROUP_SIZES).tolist()
        lone = r64['members'] == 1
        assert np.array_equal(r32['x6d'][lone], x6d[lone]) and np.array_equal(r32['betas'][lone].view(np.uint32), betas[lone].view(np.uint32))
        assert np.isnan(r64['orient'][p == 8]).all() and np.isnan(r64['orient']).sum() == 1
        assert np.array_equal(r32['x6d'][p == 8, 0], x6d[p == 8, 0])                        # an unknown d: the orientation is not fused
        assert r64['dropped'].sum() == (0 if max_deg == 0 else len(c['outliers']))
        for first in np.nonzero(np.diff(g, prepend=-1))[0]:
            n = vc.GROUP_SIZES[g[first]]
            if n > 1:
                assert (r32['x6d'][first:first + n, 1:] == r32['x6d'][first, 1:]).all() and (r32['betas'][first:first + n] == r32['betas'][first]).all()


def test_planted_truth_in_float64():
    """the planted-truth cases the GPU test runs, with the case builder's assertions: the figures of DESIGN.md section 3h"""
    f = vc.planted_reference()
    print('relative rotations from the planted ones [deg]', f['rel_err_deg'].round(3), 'residual', f['residual_deg'].round(2))
    print('clean', f['clean'], '\nreplaced, 30 deg', f['replaced_30'], '\nreplaced, plain mean', f['replaced_0'])
    assert f['rel_err_deg'].max() <= f['limit_deg'] == 1.5
    assert 0.45 < f['clean']['fused'] / f['clean']['single'] <= 0.65
    assert f['replaced_30']['dropped_elsewhere'] <= 0.01 * 200 * 23 * 3


# ---- 4. the C ABI ----
def test_view_symbols_declared_exported_and_in_the_table():
    hdr = open(os.path.join(ROOT, 'include', 'jrr.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    lib_mod, refined = _mod('_lib'), _mod('refined')
    _mod('build').build(verbose=False)
    lib = lib_mod.load()
    for name in ('jrr_view_relrot_accumulate', 'jrr_view_fuse'):
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in lib_mod.SIGNATURES and hasattr(lib, name), name
        assert re.search(r'\|[^|\n]*`' + name + r'`[^|\n]*\|', doc), name
    assert 'views.hip' in _mod('build').SOURCES and 'quat.h' in _mod('build').HEADERS
    consts = {k: int(v) for k, v in re.findall(r'\b(JRR_FUSE_[A-Z0-9_]+) = (\d+)\b', hdr)}
    assert consts == {'JRR_FUSE_MAX_VIEWS': refined.FUSE_MAX_VIEWS, 'JRR_FUSE_TILE': 32, 'JRR_FUSE_ACC_ROW': refined.FUSE_ACC_ROW,
                      'JRR_FUSE_STATUS_INDEX': 1, 'JRR_FUSE_STATUS_MARKER': 2, 'JRR_FUSE_STATUS_WIDE': 4, 'JRR_FUSE_STATUS_PAIR': 8}
    assert refined.FUSE_MAX_VIEWS == vc.MAX_VIEWS == 8 and refined.FUSE_ACC_ROW == vc.ACC_ROW == 12 and set(refined.FUSE_STATUS_BITS) == {1, 2, 4, 8}
    # the helpers moved, they were not copied
    smooth, quat = (open(os.path.join(ROOT, PKG_NAME, 'csrc', f)).read() for f in ('smooth.hip', 'quat.h'))
    for helper in ('struct Quat', 'Quat unit_quat(', 'float qdot(', 'Quat conj_mul(', 'float angle_deg('):
        assert helper in quat and helper not in smooth, helper
    # argument errors come back as a status, nothing is launched (the pointers are never read)
    import ctypes
    p, p16 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 16)
    names = ('t', 'n', 'o', 'g', 'pr', 'rp', 'np', 'm', 'b', 'c', 'a', 's', 'st')
    base = dict(t=p, n=64, o=p, g=p, pr=p, rp=p, np=4, m=40, b=0, c=0, a=p, s=p, st=None)
    relrot = lambda **kw: lib.jrr_view_relrot_accumulate(*[dict(base, **kw)[k] for k in names])
    assert relrot() == 0 and relrot(b=40) == 0                                     # an empty range launches nothing
    for k in ('t', 'o', 'g', 'pr', 'rp', 'a', 's'):
        assert relrot(**{k: None}) == -1, k
    assert relrot(b=-1) == -1 and relrot(b=41) == -1 and relrot(c=41) == -1 and relrot(b=30, c=11) == -1
    assert b'position range' in lib.jrr_last_error()
    assert relrot(b=30, c=2147483647) == -1 and relrot(n=-1) == -1 and relrot(n=1 << 31) == -1 and relrot(m=-1) == -1 and relrot(np=-1) == -1
    assert relrot(a=ctypes.c_void_p(4096 + 4)) == -1 and b'8-byte aligned' in lib.jrr_last_error()
    assert relrot(g=ctypes.c_void_p(4098)) == -1 and relrot(t=ctypes.c_void_p(4096 + 4)) == -1
    fnames = ('t', 'n', 'o', 'g', 'pr', 'r', 'np', 'm', 'chm', 'b', 'c', 'x', 'be', 'db', 'do', 'me', 'dr', 's', 'st')
    fbase = dict(t=p, n=64, o=p, g=p, pr=p, r=p16, np=4, m=40, chm=0.9, b=0, c=0, x=p16, be=p, db=p, do=p, me=p, dr=p, s=p, st=None)
    fuse = lambda **kw: lib.jrr_view_fuse(*[dict(fbase, **kw)[k] for k in fnames])
    assert fuse() == 0 and fuse(chm=0.0) == 0 and fuse(chm=-1.0) == 0
    for k in ('t', 'o', 'g', 'pr', 'r', 'x', 'be', 'db', 'do', 'me', 'dr', 's'):
        assert fuse(**{k: None}) == -1, k
    assert fuse(chm=1.5) == -1 and fuse(chm=float('nan')) == -1 and b'cos_half_max' in lib.jrr_last_error()
    assert fuse(x=ctypes.c_void_p(4096 + 8)) == -1 and b'16-byte aligned' in lib.jrr_last_error()
    assert fuse(r=ctypes.c_void_p(4096 + 8)) == -1 and fuse(me=ctypes.c_void_p(4098)) == -1 and fuse(c=41) == -1 and fuse(b=-1) == -1


def test_flags_default_to_off():
    a, refined = _mod('args'), _mod('refined')
    ns = a.get_args([])
    assert ns.fuse_refined is None and ns.fuse_max_deg == 30.0
    ns = a.get_args(['--fuse_refined', 'dir/refined_smooth.npz', '--fuse_max_deg', '0'])
    assert ns.fuse_refined == 'dir/refined_smooth.npz' and ns.fuse_max_deg == 0.0
    for k, v in a.REFERENCE_FLAGS.items():
        assert getattr(ns, k) == v, k
    src = open(os.path.join(ROOT, 'main.py')).read()
    assert src.index('args.smooth_refined') < src.index('args.fuse_refined') < src.index('optimize.optimize_pose_refiner()')
    saved = a._LazyArgs._ns
    try:
        a._LazyArgs._ns = a.get_args(['--fuse_refined', 'somewhere'])
        with pytest.raises(ValueError, match='--fuse_refined needs --data_root'):
            refined.fuse_command(log=lambda s: None)
    finally:
        a._LazyArgs._ns = saved
    assert vc.cos_half(30.0) == float(F(np.cos(np.pi / 12))) and vc.cos_half(0.0) == 0.0


# ---- 5. the files, with the three operators restated on the host ----
def _host_operators(monkeypatch):
    """engine.view_relrot_accumulate / view_fuse / pose_export on CPU tensors by the float32 restatement (the GPU tests hold the kernels to
    it)"""
    engine = _mod('engine')

    def view_relrot_accumulate(table, order, group, pair, ref_pair, acc, status, begin=0, count=None):
        x6d, _ = vc.positions_of(table.numpy(), order.numpy())
        acc += T(vc.accumulate_table(x6d, group.numpy(), pair.numpy(), ref_pair.numpy()))
        return acc

    def view_fuse(table, order, group, pair, rel, cos_half_max, status, begin=0, count=None, out=None):
        x6d, betas = vc.positions_of(table.numpy(), order.numpy())
        r = vc.fuse(x6d, betas, group.numpy(), pair.numpy(), rel.numpy(), cos_half_max, F)
        return tuple(T(np.ascontiguousarray(r[k])) for k in ('x6d', 'betas', 'body', 'orient', 'members', 'dropped'))

    def pose_export(x6d, betas, cam, index, table, status, extra=None):
        assert (table[index, 229] == 0).all()                                       # the caller cleared the markers of the rows it lists
        table[index] = T(rc.host_rows(x6d.numpy(), betas.numpy(), cam.numpy(), None if extra is None else extra.numpy()))

    for f in (view_relrot_accumulate, view_fuse, pose_export):
        monkeypatch.setattr(engine, f.__name__, f)


def _write_table(directory):
    """DIR/refined.npz + meta.json holding vc.table_case (the axis-angle part consistent with the 6-D part); (arrays, case)"""
    refined = _mod('refined')
    c = vc.table_case()
    table, order = c['table'].copy(), c['order']
    x6d, betas = vc.positions_of(table, order)
    table[order] = rc.host_rows(x6d, betas, table[order, 226:229], table[order, 230:237])
    t = refined.RefinedTable(vc.N_ROWS, 'cpu')
    t.table.copy_(T(table))
    return t.finish(directory, {'inner_iters': 3, 'data': 'dataset'}), c


def _cams_frames(c):
    """(cameras, frames) per table row that make view_groups return exactly the case's lists"""
    cams, frames = np.full(vc.N_ROWS, 99), np.full(vc.N_ROWS, -1)
    cams[c['order']], frames[c['order']] = c['pair'], c['group'] * 5
    return cams, frames


def test_fused_files_round_trip_through_load(tmp_path, monkeypatch):
    refined = _mod('refined')
    _host_operators(monkeypatch)
    out_dir = str(tmp_path / 'ref')
    raw, c = _write_table(out_dir)
    order, group, pair = c['order'], c['group'], c['pair']
    raw_bytes = open(os.path.join(out_dir, 'refined.npz'), 'rb').read()
    meta_before = json.load(open(os.path.join(out_dir, 'meta.json')))
    keys = _cams_frames(c)
    lists = refined.view_groups(keys, raw['has_refined'])
    assert np.array_equal(lists[0], order) and np.array_equal(lists[1], group) and np.array_equal(lists[2], pair)
    out = refined.fuse_views(out_dir, keys, max_deg=30.0, device='cpu',
                             rescore=lambda a, b: ({'mpjpe_eval_mm_fused': b['mpjpe_mm'] + 1}, {'mpjpe_eval_mm_fused_mean': 7.5}))
    assert sorted(os.listdir(out_dir)) == ['meta.json', 'refined.npz', 'refined_fused.npz']
    assert open(os.path.join(out_dir, 'refined.npz'), 'rb').read() == raw_bytes      # the input is not rewritten
    back = refined.load(out_dir, n=vc.N_ROWS, name='refined_fused.npz')
    meta = back.pop('meta')
    new = {'view_group', 'n_views', 'view_pair', 'fuse_delta_body_deg', 'fuse_delta_orient_deg', 'fuse_dropped', 'mpjpe_eval_mm_fused'}
    assert set(back) == set(raw) | new and all(np.array_equal(back[k], out[k], equal_nan=True) for k in back)
    # the records: the restatement's, at their rows; cam, the extras and the unlisted rows as they were
    x6d, betas = vc.positions_of(refined.pack(raw), order)
    rel, residual = vc.solve(*vc.accumulate(x6d, group, pair, c['ref_pair'], F), c['ref_pair'])
    want = vc.fuse(x6d, betas, group, pair, rel, vc.cos_half(30.0), F)
    assert np.array_equal(back['pose6d'][order], want['x6d']) and np.array_equal(back['shape'][order], want['betas'])
    assert np.array_equal(back['pose'][order], rc.log_map(rc.rot6d(want['x6d'].reshape(-1, 6), F), F).reshape(vc.M, 72))
    assert np.array_equal(back['cam'].view(np.uint32), raw['cam'].view(np.uint32)) and np.array_equal(back['has_refined'], raw['has_refined'])
    for name in refined.EXTRA_NAMES + ('mpjpe_mm', 'pampjpe_mm'):
        assert np.array_equal(back[name], raw[name], equal_nan=True), name
    rest = np.setdiff1d(np.arange(vc.N_ROWS), order)
    assert not back['pose6d'][rest].any() and np.isnan(back['fuse_delta_body_deg'][rest]).all() and np.isnan(back['fuse_delta_orient_deg'][rest]).all()
    assert (back['view_group'][rest] == -1).all() and (back['n_views'][rest] == -1).all() and (back['view_pair'][rest] == -1).all()
    assert not back['fuse_dropped'][rest].any() and back['fuse_dropped'].dtype == np.int32 and back['view_group'].dtype == np.int32
    assert np.array_equal(back['view_group'][order], group) and np.array_equal(back['view_pair'][order], pair)
    assert np.array_equal(back['n_views'][order], np.repeat(vc.GROUP_SIZES, vc.GROUP_SIZES)) and np.array_equal(back['fuse_dropped'][order], want['dropped'])
    assert np.array_equal(back['fuse_delta_body_deg'][order], want['body']) and np.array_equal(back['fuse_delta_orient_deg'][order], want['orient'], equal_nan=True)
    s = meta['fuse']
    assert s['max_deg'] == 30.0 and s['positions'] == vc.M and s['groups'] == len(vc.GROUP_SIZES) and s['duplicates'] == 0
    assert s['views_per_group_histogram'] == {'1': 1, '2': 1, '3': 1, '4': 10, '8': 3} and s['mpjpe_eval_mm_fused_mean'] == 7.5
    assert [(p['scene'], p['camera'], p['reference']) for p in s['pairs']] == [('0', str(k), k == 0) for k in range(9)]
    count = vc.accumulate(x6d, group, pair, c['ref_pair'], F)[0]
    assert [p['count'] for p in s['pairs']] == count.tolist() and s['pairs'][8]['residual_deg'] is None and s['pairs'][8]['d_axis_angle_deg'] == [0, 0, 0]
    for k in range(1, 8):                                                           # d as axis-angle in degrees: back to the quaternion
        aa = np.radians(np.array(s['pairs'][k]['d_axis_angle_deg']))
        th = np.linalg.norm(aa)
        assert np.abs(np.concatenate([[np.cos(th / 2)], np.sin(th / 2) * aa / th]) - rel[k]).max() < 1e-6
        np.testing.assert_allclose(s['pairs'][k]['residual_deg'], residual[k], rtol=1e-9)
    np.testing.assert_allclose(s['fuse_delta_body_deg_mean'], np.nanmean(back['fuse_delta_body_deg'].astype(np.float64)), rtol=1e-12)
    np.testing.assert_allclose(s['dropped_share'], want['dropped'].sum() / (24.0 * vc.M), rtol=1e-12)
    assert s['dropped_share'] > 0 and s['fuse_delta_orient_deg_mean'] > 0
    assert {k: v for k, v in meta.items() if k != 'fuse'} == meta_before and 'fuse' not in meta_before
    # the plain load still reads refined.npz; the plain mean drops nothing; the fused file can be fused again, by its name
    assert np.array_equal(refined.load(out_dir)['pose6d'], raw['pose6d'])
    plain = refined.fuse_views(out_dir, keys, max_deg=0.0, device='cpu')
    assert not plain['fuse_dropped'].any() and plain['meta']['fuse']['max_deg'] == 0.0 and 'mpjpe_eval_mm_fused' not in plain
    again = refined.fuse_views(os.path.join(out_dir, 'refined_fused.npz'), keys, device='cpu')
    assert 'fuse_delta_body_deg' in again and np.nanmax(again['fuse_delta_body_deg']) < np.nanmax(plain['fuse_delta_body_deg'])
    assert open(os.path.join(out_dir, 'refined.npz'), 'rb').read() == raw_bytes
    with pytest.raises(ValueError, match='max_deg'):
        refined.fuse_views(out_dir, keys, max_deg=-1.0, device='cpu')


def test_command_refuses_a_split_without_paths_or_of_another_length(tmp_path, monkeypatch):
    a, refined = _mod('args'), _mod('refined')
    _host_operators(monkeypatch)
    out_dir = str(tmp_path / 'ref')
    _write_table(out_dir)
    root = str(tmp_path / 'data')
    loc = os.path.join(root, 'precomputed_val')
    os.makedirs(loc)
    n = vc.N_ROWS - 1
    g = torch.Generator().manual_seed(1)
    files = dict(bboxes=torch.tensor([[100., 200., 700., 600.]]).repeat(n, 1), betas=torch.randn(n, 10, generator=g),
                 estimated_translation=torch.randn(n, 3, generator=g), gt_j2d=torch.rand(n, 17, 2, generator=g) * 1000,
                 gt_j3d=torch.randn(n, 17, 3, generator=g) * 300, intrinsics=torch.eye(3).repeat(n, 1, 1),
                 orient=torch.randn(n, 1, 6, generator=g), pose=torch.randn(n, 23, 6, generator=g))
    for k, v in files.items():
        torch.save(v, os.path.join(loc, f'{k}.pt'))
    saved = a._LazyArgs._ns
    try:
        a._LazyArgs._ns = a.get_args(['--fuse_refined', out_dir, '--data_root', root])
        with pytest.raises(FileNotFoundError, match='images.pkl'):
            refined.fuse_command(log=lambda s: None)
        with open(os.path.join(loc, 'images.pkl'), 'wb') as f:
            pickle.dump([_path('Walking', '1', k) for k in range(n)], f)
        with pytest.raises(ValueError, match='the table holds 96 samples, the split 95 with 95 frame paths'):
            refined.fuse_command(log=lambda s: None)
        os.environ['RANK'] = '1'                                                   # one process: another rank returns at once
        try:
            assert refined.fuse_command(log=lambda s: None) is None
        finally:
            del os.environ['RANK']
    finally:
        a._LazyArgs._ns = saved
