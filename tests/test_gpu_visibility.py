"""`--visible_refined` on the GPU (pytest -m gpu): jrr_point_visibility against the float64 restatement (tests/visibility_cases.py), its
independence of batch, column and launch tiling, NaN poses and defective faces, every refused argument, jrr_visibility_accumulate word
for word, and the command against the run of the same table with the host restatement in the operators' place.

What is compared.  Bit 0 of a code: equal at every query that is sure (visibility_cases: the float64 decision is the same under the
strict and the loose shift, TAU = 1e-3 on the barycentrics, 0.1 mm on the depth); the full count: equal at every query whose strict
and loose counts agree.  Bits 1 and 2: equal everywhere -- the header promises the float32 pixel operation for operation.  The caps on
what a case may leave out (1 % of the bits, 2 % of the counts, 2 of 17 joints) are asserted on the float64 numbers in
tests/test_visibility.py; this file prints what the GPU gave inside the band.  The tables are integers: equal or not.

Shapes: triangle soups of 1, 3, 4, 5 and 20 faces against 1, 63, 64, 65 and 1025 queries (a second, ragged block of 256) at batch 1, 3
and 65, and 3 x 6890 vertices + 3 x 17 joints over the body's 13 776 faces (54 chunks of 256 faces, the last ragged; 27 blocks)."""
import ctypes
import importlib
import json
import os
import pickle

import numpy as np
import pytest
import torch

import place_cases as plc
import visibility_cases as vc
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
F32, F64 = np.float32, np.float64


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _dev(a, dtype=None):
    return None if a is None else T(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _gpu(verts, faces, points, K, rect, margin=vc.MARGIN, minc=1, want_count=True):
    """-> count (B,P) or None, code (B,P), status"""
    eng = _mod('engine')
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    count, code = eng.point_visibility(_dev(verts, F32), _dev(faces, np.int32), _dev(points, F32), _dev(K, F32), _dev(rect, F32), margin, minc, status,
                                       want_count=want_count)
    torch.cuda.synchronize()
    return (None if count is None else count.cpu().numpy()), code.cpu().numpy(), int(status.item())


def _check(what, ref, count, code):
    """count and code against the float64 dict `ref`: bits 1 and 2 everywhere, bit 0 and the count where float64 is sure"""
    sb, sc = ref['sure_bit'], ref['sure_count']
    print(f'{what} {code.shape}: inside the band the GPU differs from float64 at {int((code[~sb] != ref["code"][~sb]).sum())} of {int((~sb).sum())} bits, '
          f'{int((count[~sc] != ref["count"][~sc]).sum())} of {int((~sc).sum())} counts')
    assert code.shape == ref['code'].shape and code.dtype == np.uint8 and count.dtype == np.int32
    assert np.array_equal(code & 6, ref['code'] & 6)
    assert np.array_equal(code[sb], ref['code'][sb])
    assert np.array_equal(count[sc], ref['count'][sc])


# ---- 1. against float64 ----
@pytest.mark.parametrize('shape', vc.SOUP_SHAPES)
def test_triangle_soups_against_float64(shape):
    c = vc.soup(*shape)
    count, code, status = _gpu(c['verts'], c['faces'], c['points'], c['K'], c['rect'])
    assert status == 0
    _check(f'soup {shape}', vc.soup_reference(shape), count, code)
    # the soup's own vertices as queries: every face skipped at its three corners
    count, code, status = _gpu(c['verts'], c['faces'], None, c['K'], c['rect'])
    assert status == 0
    _check(f'soup {shape} vertices', vc.soup_reference(shape, 'f64', True), count, code)


@pytest.fixture(scope='module')
def body_gpu():
    c = vc.body_case()
    cv, kv, s1 = _gpu(c['verts'], c['faces'], None, c['K'], c['rect'])
    cj, kj, s2 = _gpu(c['verts'], c['faces'], c['joints'], c['K'], c['rect'], minc=2)
    assert s1 == 0 and s2 == 0
    return cv, kv, cj, kj


def test_body_vertices_and_joints_against_float64(body_gpu):
    cv, kv, cj, kj = body_gpu
    rv, rj = vc.body_reference()
    _check('body vertices', rv, cv, kv)
    _check('body joints', rj, cj, kj)
    assert (kv == 0).any() and (kv & 1).any() and (kv & 2).any()           # the frame cuts the body, the body hides part of itself


# ---- 2. bits ----
def test_a_pose_keeps_its_bits_alone_in_a_batch_and_behind_a_nan_pose(body_gpu):
    c = vc.body_case()
    cv, kv, _, _ = body_gpu
    one = _gpu(c['verts'][1:2], c['faces'], None, c['K'][1:2], c['rect'][1:2])
    assert np.array_equal(one[0], cv[1:2]) and np.array_equal(one[1], kv[1:2])
    verts = c['verts'][[0, 1]].copy()
    verts[0] = np.nan
    two = _gpu(verts, c['faces'], None, c['K'][:2], c['rect'][:2])
    assert np.array_equal(two[0][1], cv[1]) and np.array_equal(two[1][1], kv[1]) and two[2] == 0
    assert (two[1][0] == vc.INVALID).all() and (two[0][0] == 0).all()      # the NaN pose: every query invalid, nothing counted


def test_vertices_as_points_with_the_skip_done_by_the_test(body_gpu):
    """points NULL == the vertices passed as points, minus the crossings of the faces that name the query (computed on their own: the
    query against its few faces, as points)"""
    c = vc.soup(20, 64, 3)
    count, code, _ = _gpu(c['verts'], c['faces'], None, c['K'], c['rect'])
    # the same vertices as points against the mesh WITHOUT the query's own face: one call per face left out
    want = np.zeros_like(count)
    for f in range(20):
        rest = np.delete(c['faces'], f, axis=0)
        cf, _, _ = _gpu(c['verts'], rest, c['verts'], c['K'], c['rect'])
        want[:, 3 * f:3 * f + 3] = cf[:, 3 * f:3 * f + 3]
    assert np.array_equal(count, want)
    # a column range stands in other lanes and another block
    c = vc.soup(20, 1025, 3)
    whole = _gpu(c['verts'], c['faces'], c['points'], c['K'], c['rect'])
    tail = _gpu(c['verts'], c['faces'], c['points'][:, 1000:], c['K'], c['rect'])
    assert np.array_equal(tail[0], whole[0][:, 1000:]) and np.array_equal(tail[1], whole[1][:, 1000:])


def test_count_is_optional_and_the_window_too():
    c = vc.soup(20, 1025, 3)
    count, code, _ = _gpu(c['verts'], c['faces'], c['points'], c['K'], c['rect'])
    none, code2, _ = _gpu(c['verts'], c['faces'], c['points'], c['K'], c['rect'], want_count=False)
    assert none is None and np.array_equal(code, code2)
    count3, code3, _ = _gpu(c['verts'], c['faces'], c['points'], None, None)
    assert np.array_equal(count3, count) and np.array_equal(code3, code & 5) and (code & 2).any()
    # min_crossings moves bit 0 and nothing else
    for m in (2, 255):
        cm, km, _ = _gpu(c['verts'], c['faces'], c['points'], c['K'], c['rect'], minc=m)
        assert np.array_equal(cm, count) and np.array_equal(km & 1, ((count >= m) & (code != vc.INVALID)).astype(np.uint8)) and np.array_equal(km & 6, code & 6)
    assert (count >= 2).any()


def test_a_window_edge_exactly_on_a_pixel_and_a_margin_either_side():
    # (fx X) / d + cx with X = 0.25 k, d = 2, fx = 1024, cx = 512: u = 512 + 128 k exactly
    K = vc.camera(1, 1024.0, 1024.0, 512.0, 512.0)
    pts = np.array([[[0.25 * k, 0.0, 2.0] for k in range(-4, 5)]], F32)                    # u = 0, 128, ..., 1024
    v, f = np.array([[-0.05, -0.05, 1.0], [0.1, -0.05, 1.0], [-0.05, 0.1, 1.0]], F32), np.array([[0, 1, 2]], np.int32)      # around the axis, well inside
    _, code, _ = _gpu(v[None], f, pts, K, np.array([[128.0, 0.0, 896.0, 1024.0]], F32))
    assert code[0].tolist() == [2, 0, 0, 0, 1, 0, 0, 2, 2]                               # x0 <= u < x1; the middle one sits behind the square
    _, code, _ = _gpu(v[None], f, pts, K, np.array([[0.0, 512.0, 1025.0, 513.0]], F32))
    assert (code[0] & 2 == 0).all()
    _, code, _ = _gpu(v[None], f, pts, K, np.array([[0.0, 512.5, 1025.0, 513.0]], F32))
    assert (code[0] & 2 == 2).all()
    # a plane 4 mm / 6 mm in front of the query at margin 5 mm
    big = vc.square(3.0, 2.0)
    for gap, want in ((0.004, 0), (0.006, 1)):
        count, _, _ = _gpu(big[0][None], big[1], np.array([[[0.1, 0.2, 3.0 + gap]]], F32), None, None, margin=0.005)
        assert count[0, 0] == want, (gap, count)


def test_a_face_index_out_of_range_sets_the_status_and_the_others_count():
    c = vc.soup(20, 64, 3)
    good, _, _ = _gpu(c['verts'], np.delete(c['faces'], [4, 11], axis=0), c['points'], c['K'], c['rect'])
    faces = c['faces'].copy()
    faces[4, 1], faces[11, 2] = 60, -1                                   # 60 = n_verts
    count, code, status = _gpu(c['verts'], faces, c['points'], c['K'], c['rect'])
    assert status == 1 and np.array_equal(count, good)
    # a degenerate face (a corner twice) and a face with a NaN corner add nothing either
    faces = c['faces'].copy()
    faces[4, 1] = faces[4, 0]
    verts = c['verts'].copy()
    verts[:, 3 * 11 + 2, 1] = np.nan
    count, _, status = _gpu(verts, faces, c['points'], c['K'], c['rect'])
    assert status == 0 and np.array_equal(count, good)


# ---- 3. refusals ----
def test_every_refusal_returns_non_zero_with_its_message_and_touches_nothing():
    lm = _mod('_lib')
    lib, ptr, sp = lm.load(), lm.ptr, lm.stream_ptr(torch.device(DEV))
    c = vc.soup(20, 64, 3)
    B, P, V = 3, 64, 60
    verts, faces, pts, K, rect = _dev(c['verts']), _dev(c['faces']), _dev(c['points']), _dev(c['K']), _dev(c['rect'])
    count = torch.full((B, P + 1), -99, dtype=torch.int32, device=DEV)
    code = torch.full((B, P), 77, dtype=torch.uint8, device=DEV)
    status = torch.full((1,), -99, dtype=torch.int32, device=DEV)
    acc = torch.full((2 * vc.ROW + 2,), -99, dtype=torch.int64, device=DEV)
    pv = torch.full((P + 1,), -99, dtype=torch.int64, device=DEV)
    jcode = torch.zeros((B, 17), dtype=torch.uint8, device=DEV)
    err = torch.ones((B, 18), device=DEV)
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)

    def vis(v=ptr(verts), batch=B, n_verts=V, f=ptr(faces), n_faces=20, p=ptr(pts), n_points=P, Km=ptr(K), r=ptr(rect), margin=0.005, minc=1,
            cnt=ptr(count), cd=ptr(code), st=ptr(status)):
        return lib.jrr_point_visibility(v, batch, n_verts, f, n_faces, p, n_points, Km, r, margin, minc, cnt, cd, st, sp)

    def accumulate(vcd=ptr(code), jcd=ptr(jcode), e=ptr(err), part=None, pst=None, group=None, batch=B, n_verts=P, n_groups=2, table=ptr(acc),
                   per_vertex=ptr(pv)):
        return lib.jrr_visibility_accumulate(vcd, jcd, e, part, pst, group, batch, n_verts, n_groups, table, per_vertex, sp)

    name = 'jrr_point_visibility: '
    refusals = [(vis, dict(v=None), name + 'bad argument'), (vis, dict(f=None), name + 'bad argument'),
                (vis, dict(cd=None), name + 'no output'), (vis, dict(st=None), name + 'no output'),
                (vis, dict(batch=-1), name + 'batch, n_faces and n_points must not be negative'), (vis, dict(n_faces=-1), 'must not be negative'),
                (vis, dict(n_points=-1), 'must not be negative'), (vis, dict(n_verts=0), 'n_verts at least 1'),
                (vis, dict(n_points=65537), name + 'more than 65536 points'),
                (vis, dict(p=None), name + 'points NULL: the queries are the vertices'),
                (vis, dict(Km=None), name + 'K and rect go together'), (vis, dict(r=None), 'K and rect go together'),
                (vis, dict(v=off(verts, 2)), name + 'misaligned pointer'), (vis, dict(cnt=off(count, 1)), 'misaligned pointer'),
                (vis, dict(r=off(rect, 2)), 'misaligned pointer'),
                (vis, dict(margin=-0.001), name + 'margin_m must be finite and not negative'), (vis, dict(margin=float('nan')), 'margin_m must be finite'),
                (vis, dict(margin=float('inf')), 'margin_m must be finite'),
                (vis, dict(minc=0), name + 'min_crossings 0: 1 .. 255'), (vis, dict(minc=256), 'min_crossings 256: 1 .. 255'),
                (accumulate, dict(vcd=None), 'jrr_visibility_accumulate: bad argument'), (accumulate, dict(jcd=None), 'bad argument'),
                (accumulate, dict(table=None), 'bad argument'), (accumulate, dict(batch=-1), 'jrr_visibility_accumulate: batch must not be negative'),
                (accumulate, dict(table=off(acc, 4)), 'jrr_visibility_accumulate: acc and per_vertex must be 8-byte aligned'),
                (accumulate, dict(per_vertex=off(pv, 4)), '8-byte aligned'), (accumulate, dict(e=off(err, 2)), '4-byte aligned'),
                (accumulate, dict(n_groups=0), 'jrr_visibility_accumulate: 0 groups'), (accumulate, dict(n_groups=1025), '1025 groups'),
                (accumulate, dict(n_verts=0), 'groups of 0 vertices'), (accumulate, dict(n_verts=65537), 'groups of 65537 vertices')]
    for fn, kw, message in refusals:
        rc = fn(**kw)
        assert rc != 0 and message in lib.jrr_last_error().decode(), (kw, rc, lib.jrr_last_error())
    torch.cuda.synchronize()

    def untouched():
        return ((count == -99).all().item() and (code == 77).all().item() and (status == -99).all().item() and (acc == -99).all().item()
                and (pv == -99).all().item())

    assert untouched()
    # batch 0 and no points: a clean no-op
    assert vis(batch=0) == 0 and vis(n_points=0) == 0 and accumulate(batch=0) == 0
    torch.cuda.synchronize()
    assert untouched()
    eng = _mod('engine')
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    empty = eng.point_visibility(verts[:0], faces, pts[:0], None, None, 0.005, 1, st)
    assert empty[0].shape == (0, P) and empty[1].shape == (0, P)
    with pytest.raises(ValueError, match='min_crossings 0'):
        eng.point_visibility(verts, faces, pts, None, None, 0.005, 0, st)
    with pytest.raises(ValueError, match='both or neither'):
        eng.point_visibility(verts, faces, pts, K, None, 0.005, 1, st)
    # no faces at all (the pointer still stands): nothing crosses
    cnt, cd = torch.full((B, P), -99, dtype=torch.int32, device=DEV), torch.full((B, P), 77, dtype=torch.uint8, device=DEV)
    assert vis(n_faces=0, cnt=ptr(cnt), cd=ptr(cd), st=ptr(st)) == 0
    torch.cuda.synchronize()
    assert (cnt == 0).all().item() and ((cd & 5 == 0) | (cd == 4)).all().item() and st.item() == 0


# ---- 4. the table ----
def _table(h, sl, acc=None, pv=None, **drop):
    eng = _mod('engine')
    n = h['vcode'].shape[1]
    acc = torch.zeros(h['n_groups'] * vc.ROW + vc.TRAILER, dtype=torch.int64, device=DEV) if acc is None else acc
    pv = torch.zeros(n, dtype=torch.int64, device=DEV) if pv is None else pv
    get = lambda k: None if drop.get(k) else _dev(h[k] if k == 'part' else h[k][sl])
    eng.visibility_accumulate(_dev(h['vcode'][sl]), _dev(h['jcode'][sl]), get('err'), get('part'), get('pose_status'), get('group'), h['n_groups'],
                              acc, None if drop.get('per_vertex') else pv)
    return acc, pv


def test_table_is_exactly_the_integer_accumulation_of_the_codes():
    h = vc.hand_made_codes()
    B = h['vcode'].shape[0]
    want, want_pv = vc.accumulate(h['vcode'], h['jcode'], h['err'], h['part'], h['pose_status'], h['group'], h['n_groups'])
    acc, pv = _table(h, slice(0, B))
    got = acc.cpu().numpy()
    print('rows:', got[:5].tolist(), got[vc.ROW:vc.ROW + 5].tolist(), 'trailer', got[-2:].tolist())
    assert np.array_equal(got, want) and np.array_equal(pv.cpu().numpy(), want_pv)
    assert got[vc.BAD] + got[vc.ROW + vc.BAD] == 9 and got[-2] == 2 and got[-1] == 1 and got[vc.COUNT] + got[vc.ROW + vc.COUNT] == B - 12
    assert got[vc.PART_ALL + 31] > 0 and got[vc.SUM_VERT_OUTSIDE] > 0 and got[vc.J_OCCLUDED:vc.J_OCCLUDED + 17].sum() > 0
    # as 5 + 1 + 17 poses in another order: the same integers
    order = np.random.RandomState(5).permutation(B)
    hp = {k: (v[order] if isinstance(v, np.ndarray) and k != 'part' else v) for k, v in h.items()}
    acc2, pv2 = _table(hp, slice(0, 5))
    _table(hp, slice(5, 6), acc2, pv2)
    _table(hp, slice(6, B), acc2, pv2)
    assert torch.equal(acc2, acc) and torch.equal(pv2, pv)
    # the NULL options
    for drop in ('err', 'part', 'pose_status', 'group', 'per_vertex'):
        args = {k: (None if k == drop else h[k]) for k in ('err', 'part', 'pose_status', 'group')}
        want, want_pv = vc.accumulate(h['vcode'], h['jcode'], args['err'], args['part'], args['pose_status'], args['group'], h['n_groups'])
        acc3, pv3 = _table(h, slice(0, B), **{drop: True})
        assert np.array_equal(acc3.cpu().numpy(), want), drop
        assert (pv3 == 0).all().item() if drop == 'per_vertex' else np.array_equal(pv3.cpu().numpy(), want_pv), drop


def test_table_of_the_body_codes(body_gpu):
    """6890 vertices per pose (27 strides of 256 threads), real part labels"""
    c = vc.body_case()
    _, kv, _, kj = body_gpu
    err = np.random.RandomState(2).uniform(10, 90, size=(3, 17)).astype(F32)
    group = np.array([1, 0, 1], np.int32)
    want, want_pv = vc.accumulate(kv, kj, err, c['part'], None, group, 2)
    h = {'vcode': kv, 'jcode': kj, 'err': err, 'part': c['part'], 'pose_status': None, 'group': group, 'n_groups': 2}
    acc, pv = _table(h, slice(0, 3), pose_status=True)
    assert np.array_equal(acc.cpu().numpy(), want) and np.array_equal(pv.cpu().numpy(), want_pv)


# ---- 5. the command ----
def _with_args(flags, fn):
    argsmod = _mod('args')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(flags + ['--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent'])
    try:
        torch.manual_seed(0)
        return fn()
    finally:
        argsmod._LazyArgs._ns = saved


def _write_split(root, tensors, paths):
    d = os.path.join(root, 'precomputed_val')
    os.makedirs(d, exist_ok=True)
    for k, v in tensors.items():
        torch.save(v, os.path.join(d, f'{k}.pt'))
    with open(os.path.join(d, 'images.pkl'), 'wb') as f:
        pickle.dump(paths, f)


def test_the_visible_refined_command_against_the_host_run_of_the_same_table(tmp_path, smpl_model_np, j_h36m_np, monkeypatch):
    """a 4-sample split in two groups: the driver writes a table, --place_refined places it on planted translations, --visible_refined
    runs on the GPU; then refined.visible runs once more on the host -- the same meshes, the float64 restatement in the operators' place
    -- into a copy of the directory, and the files are compared where float64 is sure"""
    import shutil
    n = 4
    sm, refined, eng, vr = _mod('smpl_model'), _mod('refined'), _mod('engine'), _mod('visibility_report')
    root = str(tmp_path / 'data')
    full = sm.synthetic_batch(smpl_model_np, j_h36m_np, n, seed=0)
    rng = np.random.RandomState(3)
    aa = rng.normal(0, 0.3, size=(n, 24, 3)).astype(F32)
    paths = [f'/data/h36m/S9/{"Walking 1" if i < 3 else "Eating"}/imageSequence/1/img_{i + 1:06d}.jpg' for i in range(n)]
    K = plc.cameras(n, rng)
    tensors = {'bboxes': torch.tensor([[100., 200., 700., 800.]]).repeat(n, 1), 'betas': T(full['betas']), 'estimated_translation': T(full['cam']),
               'gt_j2d': torch.rand(n, 17, 2) * 1000, 'gt_j3d': T(full['gt_j3d']), 'intrinsics': T(K), 'orient': T(aa[:, 0]),
               'pose': T(aa[:, 1:].reshape(n, 69))}
    _write_split(root, tensors, paths)
    out_dir = os.path.join(root, 'refined')
    flags = ['--batch_size', '3', '--inner_iters', '2', '--device', DEV, '--synthetic', '--data_root', root]
    _with_args(flags + ['--save_refined', out_dir], lambda: _mod('optimize').optimize_pose_refiner(log=lambda r: None))
    raw = refined.load(out_dir, n=n)
    mesh_of = _with_args(['--synthetic', '--device', DEV], lambda: refined._MeshOf(torch.device(DEV)))
    joints = mesh_of(raw, np.arange(n))[0].float().cpu().numpy()
    planted = np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n), rng.uniform(3.0, 5.0, n)], 1)
    tensors['gt_j2d'] = T(plc.project64(joints, planted, K)[0].astype(F32))
    _write_split(root, tensors, paths)
    common = ['--data_root', root, '--synthetic', '--device', DEV, '--batch_size', '3']
    _with_args(['--place_refined', out_dir] + common, lambda: refined.place_command(log=lambda s: None))
    before = {name: open(os.path.join(out_dir, name), 'rb').read() for name in sorted(os.listdir(out_dir))}
    host_dir = str(tmp_path / 'host')
    shutil.copytree(out_dir, host_dir)
    lines = []
    out = _with_args(['--visible_refined', out_dir, '--visible_frame', '1000', '700'] + common, lambda: refined.visible_command(log=lines.append))
    print(lines[0])
    assert sorted(os.listdir(out_dir)) == ['meta.json', 'place.json', 'place.md', 'refined.npz', 'refined_placed.npz', 'refined_visible.npz',
                                           'vertex_visibility.npy', 'visible.json', 'visible.md', 'visible_per_vertex.npy']
    for name, b in before.items():                                            # the other commands' files keep their bytes
        if name != 'meta.json':
            assert open(os.path.join(out_dir, name), 'rb').read() == b, name
    meta = json.load(open(os.path.join(out_dir, 'meta.json')))
    assert {k: v for k, v in meta.items() if k != 'visible'} == json.loads(before['meta.json']) and meta['visible']['counted'] == n
    assert len(lines) == 1 and lines[0].startswith(f'visibility of {n} poses (frame window, margin 5 mm, 0 left out)')
    # the host run: the meshes of the same engine, on the CPU
    host_mesh = lambda arrays, rows: tuple(t.float().cpu() for t in mesh_of(arrays, rows))
    host_mesh.name = mesh_of.name
    calls = vc.host_operators(monkeypatch, eng, F64)
    ds_gt = T(full['gt_j3d'])
    part = _mod('vertex_report').part_labels(mesh_of.lbs_weights)
    refined.visible(host_dir, T(K), ds_gt, paths, host_mesh, mesh_of.faces, part=part, n_parts=24, margin_mm=5.0, window='frame', frame=(1000, 700),
                    batch_size=3, device='cpu')
    sure_v = np.concatenate([calls[0]['sure_bit'], calls[2]['sure_bit']])   # per chunk: the vertices, then the joints
    sure_j = np.concatenate([calls[1]['sure_count'], calls[3]['sure_count']])
    sure_jb = np.concatenate([calls[1]['sure_bit'], calls[3]['sure_bit']])
    for r in calls:
        print(f'host chunk {r["code"].shape}: bit 0 left out {int((~r["sure_bit"]).sum())}, count left out {int((~r["sure_count"]).sum())}')
    assert (~sure_v).mean() <= vc.CAP_BIT and (~sure_j).sum(1).max() <= vc.CAP_JOINTS
    got, want = np.load(os.path.join(out_dir, 'vertex_visibility.npy')), np.load(os.path.join(host_dir, 'vertex_visibility.npy'))
    assert got.shape == (n, 6890) and np.array_equal(got & 6, want & 6) and np.array_equal(got[sure_v], want[sure_v])
    assert (got == 0).any() and (got & 1).any() and (got & 2).any()
    g, h = refined.load(out_dir, n=n, name=refined.VISIBLE_NAME), refined.load(host_dir, n=n, name=refined.VISIBLE_NAME)
    assert set(g) == set(h)
    for k in g:
        if k not in ('meta', 'joint_code', 'joint_crossings', 'n_vertices_seen'):
            assert np.array_equal(g[k], h[k], equal_nan=True) and g[k].dtype == h[k].dtype, k
    assert np.array_equal(g['joint_code'] & 6, h['joint_code'] & 6) and np.array_equal(g['joint_code'][sure_jb], h['joint_code'][sure_jb])
    assert np.array_equal(g['joint_crossings'][sure_j], h['joint_crossings'][sure_j])
    assert (np.abs(g['n_vertices_seen'] - h['n_vertices_seen']) <= (~sure_v).sum(1)).all() and (g['visible_status'] == 0).all()
    assert np.array_equal(g['n_vertices_seen'], (got == 0).sum(1)) and all(np.array_equal(g[k], out[k], equal_nan=True) for k in g if k != 'meta')
    doc = vr.load(out_dir)
    assert doc['groups'] == ['Eating', 'Walking'] and doc['table']['all']['n'] == n and doc['table']['groups']['Walking']['n'] == 3
    np.testing.assert_allclose(doc['table']['all']['vertices_seen'], (got == 0).mean(), rtol=1e-12)
    assert np.array_equal(np.load(os.path.join(out_dir, 'visible_per_vertex.npy')), (got == 0).sum(0))
