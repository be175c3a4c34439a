"""`--visible_refined` without a GPU: the restatement (tests/visibility_cases.py) against first principles, its float32 run against its
float64 run on the sure queries of every case with the caps on what a case may leave out, the row layout of the C ABI against its
Python mirrors, visibility_report.derive / write on a hand-made table, the flags and their errors, and the command's files through
refined.visible with the three operators replaced by the restatement."""
import importlib
import json
import os
import pickle
import re

import numpy as np
import pytest
import torch

import refined_cases as rc
import visibility_cases as vc
from conftest import PKG_NAME, ROOT

F32, F64 = np.float32, np.float64
T = torch.from_numpy


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _count(verts, faces, points, margin=vc.MARGIN, dtype=F64):
    return vc.counts(np.asarray(verts, F64), faces, None if points is None else np.asarray(points, F64), margin, dtype)[0]


# ---- 1. the restatement against first principles ----
def test_a_back_square_behind_a_front_square():
    front, back = vc.square(2.0, 0.5, 2), vc.square(4.0, 2.0, 4)          # the front one shadows |x|, |y| < 1 at depth 4
    back = (back[0] + [0.3, 0.1, 0.0], back[1])                             # off the axis: no ray through a corner or along a diagonal of the front grid
    verts, faces, _ = vc.pc.merge([front, back])
    cnt = _count(verts, faces, None)
    bv = back[0]
    inside = (np.abs(bv[:, 0]) < 0.99) & (np.abs(bv[:, 1]) < 0.99)
    outside = (np.abs(bv[:, 0]) > 1.01) | (np.abs(bv[:, 1]) > 1.01)
    assert inside.sum() == 4 and outside.sum() == 21                       # the grid of the back square: x = -1.7 .. 2.3, y = -1.9 .. 2.1
    assert (cnt[9:][inside] == 1).all() and (cnt[9:][outside] == 0).all() and (cnt[:9] == 0).all()
    # as points: the same, with nothing to skip; a point in front of both sees nothing in its way
    pts = np.array([[0.3, -0.2, 4.0], [0.3, -0.2, 3.0], [0.3, -0.2, 1.5], [1.5, 0.2, 5.0], [0.2, 0.1, 5.0]])
    assert _count(verts, faces, pts).tolist() == [1, 1, 0, 1, 2]


def test_a_plane_four_and_six_millimetres_in_front():
    v, f = vc.square(3.0, 2.0)
    for dtype in (F64, F32):
        got = [int(_count(v, f, [[0.1, 0.2, 3.0 + gap]], 0.005, dtype)[0]) for gap in (0.004, 0.006, 0.0, -0.01)]
        assert got == [0, 1, 0, 0], (dtype, got)
    assert _count(v, f, [[0.1, 0.2, 3.004]], 0.0)[0] == 1 and _count(v, f, [[0.1, 0.2, 3.004]], 0.003)[0] == 1


def test_a_sphere_from_outside_and_from_its_centre():
    c = np.array([0.3, -0.2, 5.0])
    v, f = vc.sphere_at(c, 1.0)
    r = vc.visibility(v[None].astype(F32), f, None, None, None, 0.005, 1)
    facing = np.einsum('vc,vc->v', v - c, v) / np.linalg.norm(v, axis=1)      # the normal against the ray: < 0 faces the camera
    # the band at the horizon: the mesh is flat between its vertices (edges of up to 31 degrees of arc), so a vertex up to sin(15.5 deg) = 0.27
    # beyond the smooth sphere's horizon still looks over its neighbours
    sure = r['sure_bit'][0] & (np.abs(facing) > 0.3)
    print(f'sphere(2): {int((~sure).sum())} of {v.shape[0]} vertices inside the band or at the horizon')
    assert sure.sum() >= 36 and (facing[sure] > 0).any() and np.array_equal(r['code'][0][sure] == 0, facing[sure] < 0)
    assert (r['count'][0][sure & (facing > 0)] == 1).all()                  # a far vertex: the near side crosses once
    # the centre: its own skin; two spheres in a row along the axis: the far centre sits behind three crossings
    assert _count(v, f, [c])[0] == 1
    far = c * 1.6
    v2, f2, _ = vc.pc.merge([(v, f), vc.sphere_at(far, 1.0)])
    r2 = vc.visibility(v2[None].astype(F32), f2, np.array([[c, far]], F32), None, None, 0.005, 2)
    assert r2['count'][0].tolist() == [1, 3] and r2['code'][0].tolist() == [0, 1] and r2['sure_count'].all()


def test_a_face_straddling_the_camera_plane_and_a_query_behind_the_camera():
    verts = np.array([[-1.0, -1.0, 2.5], [1.0, -1.0, 2.5], [0.0, 0.5, -0.5]])      # the third corner lies behind the camera; the plane: 2 y + z = 0.5
    faces = np.array([[0, 1, 2]], np.int32)
    # (0,-0.9,5): s = 0.5 / 3.2, the hit (0, -0.14, 0.78) inside the face, in front.  (0,-0.9,2): s = 2.5, behind the query.  (4,-0.9,5): the hit
    # at x = 0.625, outside the face (half width 0.427 there), and the pixel right of the frame.  Then behind the camera, in its plane, not finite.
    pts = np.array([[0.0, -0.9, 5.0], [0.0, -0.9, 2.0], [4.0, -0.9, 5.0], [0.0, -0.2, -3.0], [0.0, -0.9, 0.0], [np.nan, 0.0, 3.0]])
    for dtype in (F64, F32):
        r = vc.visibility(verts[None].astype(F32), faces, pts[None].astype(F32), vc.camera(1), np.array([[0, 0, 1000, 1000]], F32), 0.005, 1, dtype)
        assert r['count'][0].tolist() == [1, 0, 0, 0, 0, 0], (dtype, r['count'])
        assert r['code'][0].tolist() == [1, 0, 2, 4, 4, 4], (dtype, r['code'])
    a, b, c_ = verts
    n = np.cross(b - a, c_ - a)
    s = (a @ n) / (pts[0] @ n)
    assert 0 < s < 1 and abs(s - 0.5 / 3.2) < 1e-12


def test_a_window_edge_exactly_on_a_pixel():
    K = vc.camera(1, 1024.0, 1024.0, 512.0, 512.0)
    pts = np.array([[[0.25 * k, 0.0, 2.0] for k in range(-4, 5)]], F32)      # u = 512 + 128 k exactly, v = 512
    out = vc.pixel_outside(pts, K, np.array([[128.0, 0.0, 896.0, 1024.0]], F32))[0]
    assert out.tolist() == [True, False, False, False, False, False, False, True, True]      # x0 <= u < x1
    assert not vc.pixel_outside(pts, K, np.array([[0.0, 512.0, 1025.0, 513.0]], F32)).any()
    assert vc.pixel_outside(pts, K, np.array([[0.0, 512.5, 1025.0, 513.0]], F32)).all()
    assert vc.pixel_outside(pts, K, np.array([[0.0, np.nan, 1025.0, 513.0]], F32)).all()   # a NaN fails the comparison


# ---- 2. float32 against float64, and the caps ----
@pytest.mark.parametrize('shape', vc.SOUP_SHAPES)
def test_float32_equals_float64_on_the_sure_queries_of_the_soups(shape):
    for self_q in (False, True):
        r64, r32 = vc.soup_reference(shape, 'f64', self_q), vc.soup_reference(shape, 'f32', self_q)
        n = r64['count'].size
        nb, nc = int((~r64['sure_bit']).sum()), int((~r64['sure_count']).sum())
        print(f'soup {shape} self {self_q}: {n} queries, bit 0 left out {nb}, count left out {nc}')
        assert nb <= vc.CAP_BIT * n and nc <= vc.CAP_COUNT * n          # over the whole case: a pose of a soup holds 1 .. 1025 queries
        assert np.array_equal(r32['code'] & 6, r64['code'] & 6)
        assert np.array_equal(r32['code'][r64['sure_bit']], r64['code'][r64['sure_bit']])
        assert np.array_equal(r32['count'][r64['sure_count']], r64['count'][r64['sure_count']])
    c = vc.soup(*shape)
    if c['points'].size >= 24:
        assert (vc.soup_reference(shape)['code'].reshape(-1)[[3, 5, 6, 7]] == vc.INVALID).all()


def test_float32_equals_float64_on_the_sure_queries_of_the_body_and_the_caps_hold():
    (rv, rj), (sv, sj) = vc.body_reference('f64'), vc.body_reference('f32')
    vc.check_caps(rv, 'body vertices')
    vc.check_caps(rj, 'body joints', joints=True)
    for r64, r32 in ((rv, sv), (rj, sj)):
        assert np.array_equal(r32['code'] & 6, r64['code'] & 6)
        assert np.array_equal(r32['code'][r64['sure_bit']], r64['code'][r64['sure_bit']])
        assert np.array_equal(r32['count'][r64['sure_count']], r64['count'][r64['sure_count']])
    seen = (rv['code'] == 0).mean(1)
    print('share of the vertices seen per view:', seen.round(3).tolist(), '; joint crossings:', rj['count'].tolist())
    assert (seen > 0.1).all() and (seen < 0.6).all() and (rv['code'] & 2).any() and (rj['count'] >= 2).any()


# ---- 3. the C ABI ----
def test_row_layout_is_stated_once_and_mirrored():
    hdr = open(os.path.join(ROOT, 'include', 'jrr.h')).read()
    enum = {k: int(v) for k, v in re.findall(r'\b(JRR_VIS_[A-Z0-9_]+) = (\d+)', hdr)}
    vr, eng, refined = _mod('visibility_report'), _mod('engine'), _mod('refined')
    keys = ('ROW', 'TRAILER', 'COUNT', 'BAD', 'SUM_VERT_SEEN', 'SUM_VERT_OCCLUDED', 'SUM_VERT_OUTSIDE', 'J_SEEN', 'J_OCCLUDED', 'J_OUTSIDE', 'SUM_ERR_SEEN',
            'SUM_ERR_OCCLUDED', 'PART_SEEN', 'PART_ALL', 'PARTS')
    for mirror in (vr, vc):
        assert tuple(getattr(mirror, k) for k in keys) == tuple(enum['JRR_VIS_ACC_' + k] for k in keys)
        assert (mirror.OCCLUDED, mirror.OUTSIDE, mirror.INVALID, mirror.NJ) == (enum['JRR_VIS_OCCLUDED'], enum['JRR_VIS_OUTSIDE'], enum['JRR_VIS_INVALID'],
                                                                                enum['JRR_VIS_JOINTS'])
    assert enum['JRR_VIS_ACC_ROW'] == enum['JRR_VIS_ACC_PART_ALL'] + enum['JRR_VIS_ACC_PARTS'] and vr.LAYOUT_VERSION == enum['JRR_VIS_ACC_LAYOUT_VERSION']
    assert (eng.VIS_ACC_ROW, eng.VIS_ACC_TRAILER, eng.VIS_MAX_POINTS) == (enum['JRR_VIS_ACC_ROW'], enum['JRR_VIS_ACC_TRAILER'], enum['JRR_VIS_MAX_POINTS'])
    assert (eng.VIS_OCCLUDED, eng.VIS_OUTSIDE, eng.VIS_INVALID) == (1, 2, 4) and refined.VISIBLE_NO_POSE == vr.NO_POSE == 255
    assert vc.PLACE_BAD_BITS == int(re.search(r'JRR_PLACE_BAD_BITS = (\d+)', hdr).group(1))
    sig = _mod('_lib').SIGNATURES
    assert len(sig['jrr_point_visibility'][1]) == 15 and len(sig['jrr_visibility_accumulate'][1]) == 12
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert '`jrr_point_visibility`' in doc and '`jrr_visibility_accumulate`' in doc
    src = open(os.path.join(ROOT, PKG_NAME, 'csrc', 'vis.hip')).read()
    assert 'vis.hip' in _mod('build').SOURCES and 'float atomic' not in src and 'atomicAdd(q.' not in src      # the tables through acctab.h only
    assert not re.search(r'atomicAdd\(\s*(reinterpret_cast<\s*)?(float|double)', src)
    assert 'visible_command()' in open(os.path.join(ROOT, 'main.py')).read()


# ---- 4. the table and the report ----
def test_accumulate_derive_and_write_on_a_hand_made_table(tmp_path):
    vr = _mod('visibility_report')
    vcode = np.array([[0, 0, 1, 2, 3, 1], [0, 1, 1, 1, 0, 0], [0, 0, 4, 0, 0, 0], [0, 0, 0, 0, 0, 0]], np.uint8)
    jcode = np.zeros((4, 17), np.uint8)
    jcode[0, 3], jcode[1, 3], jcode[0, 5], jcode[1, 6] = 1, 1, 2, 3
    err = np.full((4, 17), 10.0, F32)
    err[0, 3], err[1, 3] = 30.0, 50.0
    part = np.array([0, 0, 1, 1, 40, -1], np.int32)
    t, pv = vc.accumulate(vcode, jcode, err, part, np.array([0, 8, 0, 2], np.int32), np.array([0, 1, 1, 1], np.int32), 2)
    assert t.shape == (2 * vc.ROW + 2,) and pv.tolist() == [2, 1, 0, 0, 1, 1]
    r0, r1 = t[:vc.ROW], t[vc.ROW:2 * vc.ROW]
    assert (r0[vc.COUNT], r0[vc.BAD], r1[vc.COUNT], r1[vc.BAD]) == (1, 0, 1, 2) and t[-2:].tolist() == [0, 0]
    assert r0[[vc.SUM_VERT_SEEN, vc.SUM_VERT_OCCLUDED, vc.SUM_VERT_OUTSIDE]].tolist() == [2, 3, 2]
    assert r0[vc.J_OCCLUDED + 3] == 1 and r0[vc.J_OUTSIDE + 5] == 1 and r0[vc.J_SEEN + 5] == 0 and r0[vc.SUM_ERR_OCCLUDED + 3] == 30 << 24
    assert r1[vc.J_OUTSIDE + 6] == 1 and r1[vc.J_OCCLUDED + 6] == 0 and r1[vc.SUM_ERR_OCCLUDED + 6] == 0 and r1[vc.SUM_ERR_SEEN + 6] == 0
    assert r0[vc.PART_ALL:vc.PART_ALL + 32].tolist() == [2, 2] + [0] * 29 + [2] and r0[vc.PART_SEEN:vc.PART_SEEN + 2].tolist() == [2, 0]
    assert vc.fixed24(F32([1.0, 0.5, 2.0 ** -24])).tolist() == [1 << 24, 1 << 23, 1]
    doc = vr.derive(t, ['a', 'b'])
    a, g0 = doc['all'], doc['groups']['a']
    assert a['n'] == 2 and a['n_bad'] == 2 and g0['vertices_seen'] == 2 / 6 and g0['vertices_occluded'] == 0.5 and a['vertices_seen'] == 5 / 12
    assert a['joints_occluded'][3] == 1.0 and a['err_occluded_per_joint_mm'][3] == 40.0 and a['err_seen_per_joint_mm'][3] is None
    assert a['err_seen_per_joint_mm'][0] == 10.0 and a['joints_outside'][5] == 0.5 and a['parts_seen'][:2] == [0.75, 0.0] and a['parts_seen'][5] is None
    empty = vr.derive(np.zeros(vc.ROW + 2, np.int64), ['all'])['all']
    assert empty['vertices_seen'] is None and empty['err_seen_mm'] is None and empty['joints_seen'] == [None] * 17
    with pytest.raises(RuntimeError, match='outside'):
        vr.derive(vc.accumulate(vcode, jcode, err, part, None, np.array([0, 2, 0, 0], np.int32), 2)[0], ['a', 'b'])
    out = str(tmp_path / 'rep')
    written = vr.write(out, doc, ['a', 'b'], 'action', 5.0, 'frame', (1000, 1000), 'initial', [('Pelvis', 2), ('L_Hip', 2)], 0)
    assert sorted(os.listdir(out)) == ['visible.json', 'visible.md'] and vr.load(out) == json.loads(json.dumps(written))
    md = open(os.path.join(out, 'visible.md'), encoding='utf-8').read()
    assert '| a | 1 | 0 | 33.3 | 50.0 | 33.3 |' in md and '| L_Hip | 2 | 0.0 |' in md and md.rstrip().endswith(vr.summary_line(written))
    assert vr.summary_line(written).startswith('visibility of 2 poses (frame window, margin 5 mm, 2 left out): vertices seen 41.7 %')


# ---- 5. the flags ----
def _write_split(root, n):
    loc = os.path.join(root, 'precomputed_val')
    os.makedirs(loc)
    g = torch.Generator().manual_seed(1)
    files = dict(bboxes=torch.tensor([[100., 200., 700., 600.]]).repeat(n, 1), betas=torch.randn(n, 10, generator=g),
                 estimated_translation=torch.randn(n, 3, generator=g), gt_j2d=torch.rand(n, 17, 2, generator=g) * 1000,
                 gt_j3d=torch.randn(n, 17, 3, generator=g) * 300, intrinsics=torch.eye(3).repeat(n, 1, 1),
                 orient=torch.randn(n, 1, 6, generator=g), pose=torch.randn(n, 23, 6, generator=g))
    for k, v in files.items():
        torch.save(v, os.path.join(loc, f'{k}.pt'))


N_ROWS = 8


def _write_table(directory, placed=True, seed=4):
    """DIR/refined.npz + meta.json of 8 rows -- row 2 without a refined pose, row 5 refined but not placed (status 4, NaN) -- and, with
    `placed`, DIR/refined_placed.npz as --place_refined leaves it: the six other rows carry the translations that put the bodies of
    visibility_cases.body_case() (each twice) where that case has them"""
    refined = _mod('refined')
    rng = np.random.RandomState(seed)
    x6d, betas, cam = rng.normal(size=(N_ROWS, 24, 6)).astype(F32), rng.normal(size=(N_ROWS, 10)).astype(F32), rng.normal(size=(N_ROWS, 3)).astype(F32)
    table = rc.host_rows(x6d, betas, cam, rng.uniform(size=(N_ROWS, 7)).astype(F32))
    table[2] = 0
    t = refined.RefinedTable(N_ROWS, 'cpu')
    t.table.copy_(T(table))
    raw = t.finish(directory, {'inner_iters': 3, 'data': 'dataset'})
    trans = np.tile(np.array([0.1, -0.05, 4.0]), (N_ROWS, 1)) + rng.uniform(-0.05, 0.05, size=(N_ROWS, 3))
    status = np.zeros(N_ROWS, np.int32)
    trans[[2, 5]], status[2], status[5] = np.nan, -1, 4
    if placed:
        np.savez(os.path.join(directory, refined.PLACE_NAME), **{k: v for k, v in raw.items() if k != 'meta'}, trans=trans, place_status=status)
    return raw, trans, status


def test_flags_and_every_flag_error(tmp_path):
    a, refined = _mod('args'), _mod('refined')
    ns = a.get_args([])
    assert ns.visible_refined is None and ns.visible_margin_mm == 5.0 and ns.visible_window == 'frame' and ns.visible_frame == [1000, 1000]
    ns = a.get_args(['--visible_refined', 'dir/refined_placed.npz', '--visible_margin_mm', '2.5', '--visible_window', 'crop', '--visible_frame', '1920', '1080'])
    assert ns.visible_refined == 'dir/refined_placed.npz' and ns.visible_margin_mm == 2.5 and ns.visible_window == 'crop' and ns.visible_frame == [1920, 1080]
    for k, v in a.REFERENCE_FLAGS.items():
        assert getattr(ns, k) == v, k
    with pytest.raises(SystemExit):
        a.build_parser().parse_args(['--visible_window', 'image'])
    # the flags stay in the records of flags the other commands write, as every flag before --place_refined does
    assert {'visible_refined', 'visible_margin_mm', 'visible_window', 'visible_frame'} <= set(vars(a.recorded(ns)))
    out_dir, root = str(tmp_path / 'ref'), str(tmp_path / 'data')
    _write_table(out_dir, placed=False)
    os.makedirs(root)
    _write_split(root, N_ROWS - 1)
    saved = a._LazyArgs._ns
    run = lambda flags: (setattr(a._LazyArgs, '_ns', a.get_args(flags)), refined.visible_command(log=lambda s: None))[1]
    try:
        with pytest.raises(ValueError, match='--visible_refined needs --data_root'):
            run(['--visible_refined', out_dir])
        for flags, message in ((['--visible_margin_mm', '-1'], '--visible_margin_mm -1.0: finite and not negative'),
                               (['--visible_margin_mm', 'nan'], '--visible_margin_mm nan'), (['--visible_frame', '0', '1000'], r'--visible_frame \[0, 1000\]')):
            with pytest.raises(ValueError, match=message):
                run(['--visible_refined', out_dir, '--data_root', root] + flags)
        with pytest.raises(FileNotFoundError, match='refined_placed.npz is missing: --place_refined writes it'):
            run(['--visible_refined', out_dir, '--data_root', root])
        with pytest.raises(ValueError, match='holds no trans: run --place_refined'):      # a table nobody placed
            run(['--visible_refined', os.path.join(out_dir, 'refined.npz'), '--data_root', root])
        _write_table(out_dir, placed=True)
        with pytest.raises(FileNotFoundError, match='images.pkl'):
            run(['--visible_refined', out_dir, '--data_root', root])
        with open(os.path.join(root, 'precomputed_val', 'images.pkl'), 'wb') as f:
            pickle.dump([f'/data/S9/Walking/imageSequence/1/img_{k:06d}.jpg' for k in range(N_ROWS - 1)], f)
        with pytest.raises(ValueError, match='the table holds 8 samples, the split 7 with 7 frame paths'):
            run(['--visible_refined', out_dir, '--data_root', root])
        os.environ['RANK'] = '1'                                                          # one process: another rank returns at once
        try:
            assert refined.visible_command(log=lambda s: None) is None
        finally:
            del os.environ['RANK']
    finally:
        a._LazyArgs._ns = saved
    assert sorted(os.listdir(out_dir)) == ['meta.json', 'refined.npz', 'refined_placed.npz']


# ---- 6. the files, with the operators restated on the host ----
def test_visible_files_on_six_bodies_in_two_groups(tmp_path, monkeypatch):
    refined, vr = _mod('refined'), _mod('visibility_report')
    vc.host_operators(monkeypatch, _mod('engine'))
    out_dir = str(tmp_path / 'ref')
    raw, trans, pstatus = _write_table(out_dir)
    c = vc.body_case()
    body = np.array([0, 1, 0, 2, 1, 0, 2, 0])                               # the body of every row (rows 2 and 5 are never asked for)
    verts_model = (c['verts'][body].astype(F64) - np.nan_to_num(trans)[:, None]).astype(F32)
    joints_model = (c['joints'][body].astype(F64) - np.nan_to_num(trans)[:, None]).astype(F32)
    asked = []

    def mesh_of(arrays, rows):
        asked.extend(int(r) for r in rows)
        return T(joints_model[rows]), T(verts_model[rows])
    mesh_of.name = 'stand-in regressor'
    K = vc.camera(N_ROWS)
    gt = ((joints_model - joints_model[:, :1]) * 1000 + np.random.RandomState(1).normal(0, 20, size=(N_ROWS, 17, 3))).astype(F32)
    paths = [f'/data/h36m/S9/{"Walking 1" if i < 4 else "Eating 2"}/imageSequence/1/img_{i + 1:06d}.jpg' for i in range(N_ROWS)]
    before = {n: open(os.path.join(out_dir, n), 'rb').read() for n in ('refined.npz', 'refined_placed.npz')}
    meta_before = json.load(open(os.path.join(out_dir, 'meta.json')))
    out = refined.visible(out_dir, K, gt, paths, mesh_of, c['faces'], part=c['part'], n_parts=24, margin_mm=5.0, window='frame', frame=(1000, 600),
                          batch_size=3, device='cpu')
    assert asked == [0, 1, 3, 4, 5, 6, 7]
    assert sorted(os.listdir(out_dir)) == ['meta.json', 'refined.npz', 'refined_placed.npz', 'refined_visible.npz', 'vertex_visibility.npy', 'visible.json',
                                           'visible.md', 'visible_per_vertex.npy']
    assert all(open(os.path.join(out_dir, n), 'rb').read() == b for n, b in before.items())      # neither input is rewritten
    codes = np.load(os.path.join(out_dir, 'vertex_visibility.npy'))
    assert codes.dtype == np.uint8 and codes.shape == (N_ROWS, 6890) and (codes[[2, 5]] == 255).all()
    good = np.array([0, 1, 3, 4, 6, 7])
    vcam = (T(verts_model[good]).float() + T(trans[good]).float()[:, None]).numpy()
    jcam = (T(joints_model[good]).float() + T(trans[good]).float()[:, None]).numpy()
    rect = np.tile(F32([0, 0, 1000, 600]), (6, 1))
    want_v = vc.visibility(vcam, c['faces'], None, K[good], rect, 0.005, 1, F32)
    want_j = vc.visibility(vcam, c['faces'], jcam, K[good], rect, 0.005, 2, F32)
    assert np.array_equal(codes[good], want_v['code']) and set(np.unique(codes[good])) == {0, 1, 2, 3}
    back = refined.load(out_dir, n=N_ROWS, name=refined.VISIBLE_NAME)
    meta = back.pop('meta')
    placed_arrays = dict(np.load(os.path.join(out_dir, 'refined_placed.npz')))
    assert set(back) == set(placed_arrays) | {'joint_code', 'joint_crossings', 'n_vertices_seen', 'visible_status'}
    assert all(np.array_equal(back[k], placed_arrays[k], equal_nan=True) for k in placed_arrays)      # every array of the input, unchanged
    assert all(np.array_equal(back[k], out[k], equal_nan=True) for k in back)
    assert back['joint_code'].dtype == np.uint8 and back['joint_crossings'].dtype == np.int32 and back['n_vertices_seen'].dtype == np.int32
    assert np.array_equal(back['joint_code'][good], want_j['code']) and np.array_equal(back['joint_crossings'][good], want_j['count'])
    assert (back['joint_code'][[2, 5]] == 255).all() and (back['joint_crossings'][[2, 5]] == -1).all() and (back['n_vertices_seen'][[2, 5]] == -1).all()
    assert np.array_equal(back['n_vertices_seen'][good], (want_v['code'] == 0).sum(1))
    assert back['visible_status'].tolist() == [0, 0, -1, 0, 0, 1, 0, 0]
    pv = np.load(os.path.join(out_dir, 'visible_per_vertex.npy'))
    assert pv.dtype == np.int64 and np.array_equal(pv, (want_v['code'] == 0).sum(0))
    # the report: recounted from the files
    doc = vr.load(out_dir)
    assert doc['groups'] == ['Eating', 'Walking'] and doc['window'] == 'frame' and doc['frame'] == [1000, 600] and doc['margin_mm'] == 5.0
    assert doc['j_regressor'] == 'stand-in regressor' and doc['parts'][0][0] == 'Pelvis' and len(doc['parts']) == 24 and doc['face_index_status'] == 0
    a, w, e = doc['table']['all'], doc['table']['groups']['Walking'], doc['table']['groups']['Eating']
    assert (a['n'], a['n_bad'], w['n'], w['n_bad'], e['n'], e['n_bad']) == (6, 1, 3, 0, 3, 1)
    np.testing.assert_allclose(a['vertices_seen'], (codes[good] == 0).mean(), rtol=1e-12)
    np.testing.assert_allclose(a['vertices_occluded'], (codes[good] & 1).mean(), rtol=1e-12)
    np.testing.assert_allclose(w['vertices_outside'], ((codes[[0, 1, 3]] >> 1) & 1).mean(), rtol=1e-12)
    jc = back['joint_code'][good]
    assert a['joints_seen_n'] == (jc == 0).sum(0).tolist() and a['joints_occluded_n'] == ((jc & 3) == 1).sum(0).tolist()
    err = np.linalg.norm((jcam - jcam[:, :1]).astype(F64) * 1000 - (gt[good] - gt[good][:, :1]), axis=2)      # the command centres the ground truth
    if (jc == 0).any():
        np.testing.assert_allclose(a['err_seen_mm'], err[jc == 0].mean(), rtol=1e-5)
    for p in range(32):                                                       # a label without a vertex has no share
        mine = c['part'] == p
        assert (a['parts_seen'][p] is None) if not mine.any() else abs(a['parts_seen'][p] - (codes[good][:, mine] == 0).mean()) < 1e-12, p
    md = open(os.path.join(out_dir, 'visible.md'), encoding='utf-8').read()
    assert '| Walking | 3 | 0 |' in md and '| R_Wrist |' in md and '| Pelvis |' in md and md.rstrip().endswith(vr.summary_line(doc))
    assert {k: v for k, v in meta.items() if k != 'visible'} == meta_before and meta['visible']['counted'] == 6 and meta['visible']['rows'] == 7
    assert meta['visible']['placed'] == 6 and meta['visible']['source'] == 'refined_placed.npz'
    # the crop window, a named file, one group, no parts; the errors of the arrays
    bboxes = np.tile(F32([200.0, 300.0, 700.0, 700.0]), (N_ROWS, 1))        # (min_y, min_x, max_y, max_x): the square [250, 200, 750, 700]
    out2 = refined.visible(os.path.join(out_dir, refined.PLACE_NAME), K, gt, None, mesh_of, c['faces'], window='crop', bboxes=bboxes, group_kind='none',
                           device='cpu')
    assert np.array_equal(refined.visible_window('crop', N_ROWS, bboxes=T(bboxes)).numpy(), np.tile(F32([250, 200, 750, 700]), (N_ROWS, 1)))
    codes2 = np.load(os.path.join(out_dir, 'vertex_visibility.npy'))
    assert np.array_equal(codes2[good] & 1, codes[good] & 1) and not np.array_equal(codes2 & 2, codes & 2)      # the window moves bit 1 alone
    assert vr.load(out_dir)['groups'] == ['all'] and vr.load(out_dir)['parts'] is None and out2['meta']['visible']['window'] == 'crop'
    for bad, message in ((dict(intrinsics=K[:-1]), 'intrinsics should be'), (dict(gt=gt[:, :16]), 'gt_j3d should be'), (dict(paths=paths[:-1]), '7 paths'),
                         (dict(margin_mm=-1.0), 'margin_mm -1.0'), (dict(window='crop'), 'the crop window needs bboxes'), (dict(window='image'), 'frame or crop')):
        kw = dict(dict(intrinsics=K, gt=gt, paths=paths), **bad)
        with pytest.raises(ValueError, match=message):
            refined.visible(out_dir, kw.pop('intrinsics'), kw.pop('gt'), kw.pop('paths'), mesh_of, c['faces'], device='cpu', **kw)
