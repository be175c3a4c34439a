"""The depth section of the regressor report on the GPU (pytest -m gpu): jrr_point_mesh_depth against the float64 restatement
(tests/depth_cases.py), its tie rule, its independence of batch and column, NaN and defective faces, jrr_depth_accumulate word for word,
and `--regressor_report_depth` through `--eval_vertices` with one rank and with two gloo ranks on one GPU.

Bounds.  Distance and winding number: `bound(d) = 3 d + 1e-7`, d the float32 restatement's distance from the float64 one on the test's
own inputs (tests/test_joint_depth.py prints them: about 6e-8 m and 1.2e-7 to 1.9e-7).  Every test prints d, the bound and what the GPU
gave before it asserts.  Bits where the header promises bits.  The table is integers: equal or not.  A mean of the report against the
float64 restatement: the distance bound of its own points.

Shapes: batch 1, 3, 5 and 1, 17, 51, 64 points over an octahedron (8 faces: half a pass of the 16 waves), a cube (12), the
octahedron subdivided twice (128) and three times (512: whole passes) and the synthetic body (13 776 = 861 passes; 6890 vertices)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_cases as dc
from conftest import PKG_NAME, ROOT

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
F32, F64 = np.float32, np.float64


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _gpu(verts, faces, points):
    """-> dist, wind, face, status as numpy"""
    eng = _mod('engine')
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    d, w, f = eng.point_mesh_depth(T(np.ascontiguousarray(verts, dtype=F32)).to(DEV), T(np.ascontiguousarray(faces, dtype=np.int32)).to(DEV),
                                   T(np.ascontiguousarray(points, dtype=F32)).to(DEV), status)
    return d.cpu().numpy(), w.cpu().numpy(), f.cpu().numpy(), int(status.item())


def _bits(*arrays):
    return [np.ascontiguousarray(a).view(np.uint32 if a.dtype == F32 else a.dtype) for a in arrays]


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(*a), _bits(*b)))


def _check(name, got, B, P, what=''):
    """dist, wind, inside flags and the face of `got` against the float64 restatement of case `name`, poses [:B], points [:P]"""
    d, w, f = got
    r64, r32 = dc.reference(name), dc.reference(name, 'f32')
    sl = (slice(0, B), slice(0, P))
    dd = np.abs(r32['dist'][sl].astype(F64) - r64['dist'][sl]).max()
    dw = np.abs(r32['wind'][sl].astype(F64) - r64['wind'][sl]).max()
    ed, ew = np.abs(d.astype(F64) - r64['dist'][sl]).max(), np.abs(w.astype(F64) - r64['wind'][sl]).max()
    print(f'{name} B {B} P {P}{what}: dist d {dd:.2e} bound {dc.bound(dd):.2e} gpu {ed:.2e} m;  wind d {dw:.2e} bound {dc.bound(dw):.2e} gpu {ew:.2e}')
    assert ed <= dc.bound(dd) and ew <= dc.bound(dw)
    assert np.array_equal(dc.inside(w), dc.inside(r64['wind'][sl]))
    assert f.min() >= 0 and f.max() < r64['all'].shape[2]
    attained = np.take_along_axis(r64['all'][sl], f[..., None].astype(np.int64), axis=2)[..., 0]
    assert (attained <= r64['dist'][sl] + dc.bound(dd)).all()


# ---- 1. against float64 ----
@pytest.mark.parametrize('P', [1, 17, 51, 64])
@pytest.mark.parametrize('B', [1, 3, 5])
@pytest.mark.parametrize('name', dc.CONVEX)
def test_convex_meshes_against_float64(name, B, P):
    v, f, p = dc.case(name)
    d, w, fc, status = _gpu(v[:B], f, p[:B, :P])
    assert status == 0 and d.shape == (B, P)
    _check(name, (d, w, fc), B, P)


@pytest.mark.parametrize('B,P', [(1, 1), (1, 17), (3, 51), (3, 64)])
def test_body_against_float64(B, P):
    v, f, p = dc.case('body')
    d, w, fc, status = _gpu(v[:B], f, p[:B, :P])
    assert status == 0
    _check('body', (d, w, fc), B, P)
    if P >= 17:
        assert (w[:, :17] < -0.5).all()          # the shipped joints are inside, and this body is wound inwards: -1


def test_outputs_are_optional_but_not_all_three():
    eng = _mod('engine')
    v, f, p = dc.case('cube')
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    tv, tf, tp = T(v[:3]).to(DEV), T(f).to(DEV), T(p[:3, :17].copy()).to(DEV)
    full = eng.point_mesh_depth(tv, tf, tp, status)
    for keep in range(3):
        want = [k == keep for k in range(3)]
        got = eng.point_mesh_depth(tv, tf, tp, status, *want)
        assert [g is not None for g in got] == want and torch.equal(got[keep], full[keep])
    with pytest.raises(ValueError):
        eng.point_mesh_depth(tv, tf, tp, status, False, False, False)
    assert all(t.shape == (0, 17) for t in eng.point_mesh_depth(tv[:0], tf, tp[:0], status))


# ---- 2. the tie rule ----
def test_above_a_shared_corner_the_smallest_face_index_wins():
    v, f = dc.cube()
    up = np.array([[0, 0, 0.25], [0, 0.25, 0], [0.25, 0, 0]])
    for faces in (f, dc._relabel(f), dc._relabel(f)[::-1].copy()):
        pts = np.stack([v[c] + np.sign(v[c]) * up[c % 3] for c in range(8)])[None].astype(F32)       # exact in float32
        d, w, fc, _ = _gpu(v[None], faces, pts)
        r = dc.depth(v, faces, pts[0])
        assert np.array_equal(d[0], np.full(8, 0.25, dtype=F32))
        for c in range(8):
            holders = np.flatnonzero((faces == c).any(axis=1) & (r['all'][c] == 0.25))
            assert holders.size >= 2 and fc[0, c] == holders.min(), (c, fc[0, c], holders)
    # inside one wave: faces k and k + 16 are walked by the same wave, whose strict `<` keeps the earlier.  The cube, four of its
    # faces again, then the cube again: face 16 + k repeats face k, and 12..15 repeat 0..3 in other waves
    for base in (f, dc._relabel(f)[::-1].copy()):
        faces = np.concatenate([base, base[:4], base])
        d, w, fc, _ = _gpu(v[None], faces, pts)
        r = dc.depth(v, faces, pts[0])
        assert np.array_equal(d[0], np.full(8, 0.25, dtype=F32))
        for c in range(8):
            holders = np.flatnonzero((faces == c).any(axis=1) & (r['all'][c] == 0.25))
            assert (holders.min() + 16 in holders) and fc[0, c] == holders.min(), (c, fc[0, c], holders)


# ---- 3. independence ----
@pytest.mark.parametrize('name', ['sphere3', 'body'])
def test_a_pose_gives_the_same_bits_alone_and_inside_a_batch(name):
    v, f, p = dc.case(name)
    n = v.shape[0]
    whole = _gpu(v, f, p[:, :51])[:3]
    for b in range(n):
        alone = _gpu(v[b:b + 1], f, p[b:b + 1, :51])[:3]
        assert _same_bits(alone, [x[b:b + 1] for x in whole]), b
    if n < 5:                                    # the body has three poses: five by repeating two
        idx = [0, 1, 2, 1, 0]
        five = _gpu(v[idx], f, p[idx][:, :51])[:3]
        assert _same_bits(five, [x[idx] for x in whole])


@pytest.mark.parametrize('name', ['cube', 'sphere3', 'body'])
def test_a_point_gives_the_same_bits_in_any_column(name):
    v, f, p = dc.case(name)
    v, p = v[:3], p[:3]
    alone = _gpu(v, f, p[:, 17:34])[:3]
    within = _gpu(v, f, p[:, :51])[:3]
    assert _same_bits(alone, [x[:, 17:34] for x in within])
    one = _gpu(v, f, p[:, 40:41])[:3]
    last = _gpu(v, f, p)[:3]
    assert _same_bits(one, [x[:, 40:41] for x in last])


# ---- 4. NaN ----
def test_a_nan_vertex_poisons_its_pose_and_a_nan_point_its_column():
    v, f, p = dc.case('sphere2')
    p = p[:, :17]
    clean = _gpu(v, f, p)[:3]
    bad_v = v.copy()
    bad_v[2, 65, 1] = np.nan                     # the last vertex of pose 2
    d, w, fc, status = _gpu(bad_v, f, p)
    assert np.isnan(d[2]).all() and np.isnan(w[2]).all() and (fc[2] == -1).all() and status == 0
    keep = [0, 1, 3, 4]
    assert _same_bits([d[keep], w[keep], fc[keep]], [x[keep] for x in clean])
    bad_p = p.copy()
    bad_p[1, 5, 2] = np.nan
    bad_p[3, 0, 0] = np.inf
    d, w, fc, _ = _gpu(v, f, bad_p)
    hit = np.zeros((5, 17), dtype=bool)
    hit[1, 5] = hit[3, 0] = True
    assert np.isnan(d[hit]).all() and np.isnan(w[hit]).all() and (fc[hit] == -1).all()
    assert _same_bits([d[~hit], w[~hit], fc[~hit]], [x[~hit] for x in clean])


# ---- 5. defective faces ----
def test_a_face_index_out_of_range_is_skipped_and_reported():
    v, f, p = dc.case('sphere2')
    p = p[:, :51]
    clean = _gpu(v, f, p)
    assert clean[3] == 0
    for bad in ([0, 1, 66], [-1, 2, 3], [5, 1 << 30, 7]):
        d, w, fc, status = _gpu(v, np.concatenate([f, [bad]]), p)                   # behind the others: every face keeps its partial sum
        assert status == 1 and _same_bits([d, w, fc], clean[:3]), bad
    d, w, fc, status = _gpu(v, np.concatenate([[[0, 1, 66]], f]), p)                # in front: the sums are ordered anew
    r64, r32 = dc.reference('sphere2'), dc.reference('sphere2', 'f32')
    dw = np.abs(r32['wind'][:, :51].astype(F64) - r64['wind'][:, :51]).max()
    print(f'skipped face in front: wind against the mesh without it {np.abs(w - clean[1]).max():.2e}, bound {dc.bound(dw):.2e}')
    assert status == 1 and np.array_equal(d, clean[0]) and np.array_equal(fc, clean[2] + 1) and np.abs(w - clean[1]).max() <= dc.bound(dw)


def test_a_face_without_area_changes_nothing():
    v, f, p = dc.case('cube')
    clean = _gpu(v, f, p)
    for flat in ([3, 3, 5], [2, 2, 2], [0, 1, 1]):        # a diagonal of a side, a corner, an edge: all on the surface
        d, w, fc, status = _gpu(v, np.concatenate([f, [flat]]), p)
        r64, r32 = dc.reference('cube'), dc.reference('cube', 'f32')
        dw = np.abs(r32['wind'].astype(F64) - r64['wind']).max()
        print(f'flat face {flat}: wind moved {np.abs(w - clean[1]).max():.2e}, bound {dc.bound(dw):.2e}')
        assert status == 0 and np.array_equal(d, clean[0]) and np.abs(w - clean[1]).max() <= dc.bound(dw)
        assert np.array_equal(dc.inside(w), dc.inside(clean[1]))
        _check('cube', (d, w, np.minimum(fc, 11)), 5, 64, f' + flat face {flat}')
        assert (fc <= 11).all()                  # where the flat face ties with a real one, the smaller index stays


# ---- 6. orientation ----
@pytest.mark.parametrize('name', ['sphere3', 'body'])
def test_rewound_faces_negate_the_winding_number_and_nothing_else(name):
    v, f, p = dc.case(name)
    B = v.shape[0]
    d, w, fc, _ = _gpu(v, f, p)
    d2, w2, fc2, _ = _gpu(v, f[:, ::-1].copy(), p)
    r64, r32 = dc.reference(name), dc.reference(name, 'f32')
    dd = np.abs(r32['dist'].astype(F64) - r64['dist']).max()
    dw = np.abs(r32['wind'].astype(F64) - r64['wind']).max()
    print(f'{name} re-wound: wind + wind {np.abs(w + w2).max():.2e} bound {dc.bound(dw):.2e}; dist moved {np.abs(d - d2).max():.2e} bound {dc.bound(dd):.2e}')
    assert np.abs(w.astype(F64) + w2).max() <= dc.bound(dw) and np.abs(w2.astype(F64) + r64['wind']).max() <= dc.bound(dw)
    assert np.abs(d2.astype(F64) - r64['dist']).max() <= dc.bound(dd) and np.abs(d.astype(F64) - d2).max() <= dc.bound(dd)
    assert np.array_equal(dc.inside(w), dc.inside(w2))
    assert np.sign(w[dc.inside(w)]).tolist() == (-np.sign(w2[dc.inside(w2)])).tolist()


# ---- 7. the accumulator ----
def _acc_inputs():
    v, f, p = dc.case('sphere2')
    rs = np.random.RandomState(31)
    idx = np.arange(65) % 5
    pts = p[idx][:, :51] + rs.normal(scale=0.02, size=(65, 51, 3)).astype(F32)
    pts[:, 40:] *= rs.uniform(0.0, 1.2, size=(65, 11, 1)).astype(F32)       # pulled towards the mesh and through it: depths of every sign
    pts[7, 3, 0] = np.nan                                                   # a bad pose
    group = (np.arange(65) % 3).astype(np.int32)
    group[[4, 50]] = -1
    group[[9, 33, 64]] = 3
    return v[idx], f, pts.astype(F32), group


def test_accumulate_word_for_word_in_one_call_and_in_two():
    eng = _mod('engine')
    v, f, pts, group = _acc_inputs()
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    dist, wind, _ = eng.point_mesh_depth(T(v).to(DEV), T(f).to(DEV), T(pts).to(DEV), status, want_face=False)
    g = T(group).to(DEV)
    new = lambda n: torch.zeros(n * dc.ROW + dc.TRAILER, dtype=torch.int64, device=DEV)
    one, two, none = new(3), new(3), new(1)
    eng.depth_accumulate(dist, wind, g, 3, one)
    eng.depth_accumulate(dist[:40], wind[:40], g[:40], 3, two)
    eng.depth_accumulate(dist[40:], wind[40:], g[40:], 3, two)
    eng.depth_accumulate(dist, wind, None, 1, none)
    want = dc.accumulate(dist.cpu().numpy(), wind.cpu().numpy(), group, 3)
    rows = want[:3 * dc.ROW].reshape(3, dc.ROW)
    print('counted', rows[:, dc.COUNT].tolist(), 'bad', rows[:, dc.BAD].tolist(), 'trailer', want[-2:].tolist(), 'outside', int(rows[:, dc.OUTSIDE:dc.UNSURE].sum()),
          'unsure', int(rows[:, dc.UNSURE:dc.SUM].sum()))
    assert want[-2:].tolist() == [2, 3] and rows[:, dc.BAD].sum() == 1 and rows[:, dc.COUNT].sum() == 59
    assert 0 < rows[:, dc.OUTSIDE:dc.UNSURE].sum() < 59 * 51
    assert np.array_equal(one.cpu().numpy(), want) and np.array_equal(two.cpu().numpy(), want)
    assert np.array_equal(none.cpu().numpy(), dc.accumulate(dist.cpu().numpy(), wind.cpu().numpy(), None, 1))


# ---- 8. the driver ----
SYN = ['--synthetic', '--device', DEV, '--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent']


def _with_args(flags, fn):
    argsmod = _mod('args')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(flags)
    try:
        return fn()
    finally:
        argsmod._LazyArgs._ns = saved


@pytest.fixture(scope='module')
def driver_run(tmp_path_factory):
    """the 6 meshes of depth_cases.driver_case() as an --eval_vertices directory with two groups, the retrained regressor whose R_Wrist
    lies outside the skin; the report without and then with --regressor_report_depth into the same directory"""
    tmp = str(tmp_path_factory.mktemp('joint_depth'))
    c = dc.driver_case()
    model, J, J2, V, gt, ids = c['model'], c['J'], c['J2'], c['verts'], c['gt_mm'], c['ids']
    ck = os.path.join(tmp, 'retrained_J_Regressor.pt')
    _mod('checkpoint').save_j_regressor(T(J2), ck)
    vdir = os.path.join(tmp, 'meshes')
    os.makedirs(vdir)
    np.save(os.path.join(vdir, 'vertices.npy'), V)
    np.save(os.path.join(vdir, 'gt_j3d.npy'), gt)
    np.save(os.path.join(vdir, 'group.npy'), ids)
    with open(os.path.join(vdir, 'group_names.txt'), 'w') as f:
        f.write('Walking\nSitting\n')
    flags = SYN + ['--batch_size', '4', '--eval_j_regressor', ck, '--eval_vertices', vdir, '--regressor_report_size', '64', '--regressor_report_images', '1']
    out = os.path.join(tmp, 'one')
    _with_args(flags + ['--regressor_report', out], lambda: _mod('eval_report').evaluate_vertices(log=lambda s: None))
    plain = {n: open(os.path.join(out, n), 'rb').read() for n in sorted(os.listdir(out))}
    lines = []
    _with_args(flags + ['--regressor_report', out, '--regressor_report_depth'], lambda: _mod('eval_report').evaluate_vertices(log=lines.append))
    return tmp, flags, out, plain, lines, (model, J, J2, V, gt, ids)


def test_the_flag_adds_two_files_and_changes_no_other(driver_run):
    tmp, flags, out, plain, lines, _ = driver_run
    assert 'depth.json' not in plain and 'regressor.json' in plain
    now = {n: open(os.path.join(out, n), 'rb').read() for n in sorted(os.listdir(out))}
    assert sorted(set(now) - set(plain)) == ['depth.json', 'depth.md']
    for n, data in plain.items():
        assert now[n] == data, n                 # regressor.json, regressor.md and the pictures keep their bytes
    assert any('depth.md' in s for s in lines)


def _driver_points(J, J2, V, gt):
    """the 51 points per pose as the driver forms them: both regressors on the device, the ground truth at A's pelvis"""
    eng, utils = _mod('engine'), _mod('utils')
    Js = torch.stack([T(J), T(J2)]).to(DEV)
    joints = eng.JointRegressorTable(Js, utils.find_j_reg_mask(Js[0])).regress(T(V).to(DEV))
    gtc = utils.move_pelvis(T(gt).to(DEV))
    pts = torch.cat([joints[0], joints[1], gtc / 1000.0 + joints[0][:, :1]], dim=1).cpu().numpy()
    assert np.abs(pts - dc.driver_points_host()).max() < 1e-5          # the points whose conditions tests/test_joint_depth.py asserts
    return pts


def _check_depth_doc(doc, points, V, faces, ids):
    rr = _mod('regressor_report')
    r64 = dc.depth_batch(V, faces, points, F64)
    r32 = dc.depth_batch(V, faces, points, F32)
    dd = np.abs(r32['dist'].astype(F64) - r64['dist']).max()
    tol = dc.bound(dd)
    dc.check_inside_conditions(r64)              # every point at least 1 mm from the surface: the flags are no matter of rounding
    ins = np.abs(r64['wind']) > 0.5
    signed = np.where(ins, r64['dist'], -r64['dist'])
    for name, keep in (('all', ids >= 0), ('Walking', ids == 0), ('Sitting', ids == 1)):
        r = doc['data']['all'] if name == 'all' else doc['data']['groups'][name]
        assert r['n'] == int(keep.sum()) and r['n_bad'] == 0
        for s, key in enumerate(rr.DEPTH_SETS):
            cols = slice(17 * s, 17 * s + 17)
            err = np.abs(np.array(r['sets'][key]['mean_mm']) / 1000.0 - signed[keep][:, cols].mean(0)).max()
            print(f'{name} {key}: mean depth against float64 {err:.2e} m, bound {tol:.2e} (d {dd:.2e})')
            assert err <= tol
            assert np.array_equal(np.array(r['sets'][key]['outside']), (~ins[keep][:, cols]).mean(0))
            assert np.array(r['sets'][key]['unsure']).max() == 0
            # the quantiles are bin edges: the upper edge of the 4-mm bin that holds the ceil(p n)-th smallest depth
            ordered = np.sort(signed[keep][:, cols], axis=0)
            for p, q in ((0.5, 'median_mm'), (0.05, 'p05_mm')):
                x = ordered[int(np.ceil(p * r['n'])) - 1]
                assert r['sets'][key][q] == (-64.0 + 4.0 * (np.clip(np.floor((x + 0.064) * 250.0), 0, 63) + 1)).tolist(), (name, key, q)
    return signed


def test_depth_json_against_float64_and_the_template_block(driver_run):
    tmp, flags, out, plain, lines, (model, J, J2, V, gt, ids) = driver_run
    rr, eng = _mod('regressor_report'), _mod('engine')
    doc = rr.load_depth(out)
    assert doc['groups'] == ['Walking', 'Sitting'] and doc['sets'] == list(rr.DEPTH_SETS) and doc['orientation'] == -1 and doc['data']['ignored'] == 0
    faces = np.asarray(model['faces']).astype(np.int32)
    signed = _check_depth_doc(doc, _driver_points(J, J2, V, gt), V, faces, ids)
    assert doc['newly_outside'] == [j for j in range(17) if (signed[:, 17 + j] < 0).any() and not (signed[:, j] < 0).any()]
    assert doc['newly_outside'] == [16] and doc['data']['all']['sets']['retrained']['outside'][16] == 1.0
    md = open(os.path.join(out, 'depth.md')).read()
    assert md.count('**!**') == 1 and '| R_Wrist **!** |' in md and 'outside the body in some pose and the initial one in none: R_Wrist.' in md
    assert 'winding -1 inside' in md
    # the template block is a direct call on v_template
    mask = _mod('utils').find_j_reg_mask(T(J)).numpy()
    vt = np.asarray(model['v_template'], dtype=F32)
    pts = np.concatenate([rr.normalised(Jx, mask) @ vt.astype(F64) for Jx in (J, J2)]).astype(F32)
    d, w, fc, status = _gpu(vt[None], faces, pts[None])
    depth_mm = np.where(np.abs(w[0]) > 0.5, d[0], -d[0]).astype(F64) * 1000.0
    for s, key in enumerate(('initial', 'retrained')):
        t = doc['template'][key]
        assert t['depth_mm'] == depth_mm[17 * s:17 * s + 17].tolist() and t['face'] == fc[0, 17 * s:17 * s + 17].tolist()
        assert t['wind'] == w[0, 17 * s:17 * s + 17].astype(F64).tolist()
    assert abs(min(doc['template']['initial']['depth_mm']) - 1.45) < 0.01


def test_two_gloo_ranks_write_the_same_numbers(driver_run):
    """main.py --eval_vertices --regressor_report --regressor_report_depth under torchrun, two ranks over gloo sharing cuda:0 (3 meshes each)"""
    tmp, flags, out, plain, lines, _ = driver_run
    rr = _mod('regressor_report')
    out2 = os.path.join(tmp, 'two')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1', '--master-port',
           '29591', os.path.join(ROOT, 'main.py')] + flags + ['--regressor_report', out2, '--regressor_report_depth', '--single_device',
                                                              '--dist_backend', 'gloo']
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    one, two = rr.load_depth(out), rr.load_depth(out2)
    assert two['data']['all']['n'] == 6 and two['data'] == one['data'] and two['template'] == one['template']
    assert two['newly_outside'] == one['newly_outside']


def test_the_parameter_path_writes_the_depth_section_too(driver_run):
    """test_pose_refiner_model on 2 synthetic batches of 8 poses: the vertices of its forward, the faces of its own body model"""
    tmp, flags, out, plain, lines, (model, J, J2, V, gt, ids) = driver_run
    rr = _mod('regressor_report')
    ck = flags[flags.index('--eval_j_regressor') + 1]
    out3 = os.path.join(tmp, 'parameters')
    said = []
    _with_args(SYN + ['--batch_size', '8', '--synthetic_batches', '2', '--regressor_report', out3, '--regressor_report_depth', '--regressor_report_size', '64',
                      '--regressor_report_images', '1'], lambda: _mod('test').test_pose_refiner_model(retrained_path=ck, log=said.append))
    doc = rr.load_depth(out3)
    assert doc['source'] == 'parameters' and doc['groups'] == ['all'] and doc['orientation'] == -1
    r = doc['data']['all']
    assert r['n'] == 16 and r['n_bad'] == 0 and doc['data']['ignored'] == 0
    for key in rr.DEPTH_SETS:
        assert len(r['sets'][key]['mean_mm']) == 17 and np.isfinite(r['sets'][key]['mean_mm']).all() and max(r['sets'][key]['unsure']) == 0
    assert doc['template'] == rr.load_depth(out)['template']
    assert os.path.isfile(os.path.join(out3, 'regressor.json')) and os.path.isfile(os.path.join(out3, 'depth.md'))


def test_the_flag_is_refused_without_a_body_model(driver_run):
    tmp, flags, out, plain, lines, _ = driver_run
    no_synth = [f for f in flags if f != '--synthetic']
    with pytest.raises(ValueError, match='faces of the body model'):
        _with_args(no_synth + ['--regressor_report', os.path.join(tmp, 'none'), '--regressor_report_depth'],
                   lambda: _mod('eval_report').evaluate_vertices(log=lambda s: None))
    assert not os.path.exists(os.path.join(tmp, 'none'))
