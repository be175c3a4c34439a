"""The self-penetration report on the GPU (pytest -m gpu): jrr_mesh_winding against the float64 restatement (tests/penetration_cases.py),
its independence of batch, column and launch tiling, NaN and defective faces, every refused argument, jrr_penetration_accumulate word
for word, and `--eval_penetration` through `--eval_vertices` with one rank and with two gloo ranks on one GPU.

Bounds.  Winding number: `depth_cases.bound(d) = 3 d + 1e-7`, d the float32 restatement's distance from the float64 one on the case's
own inputs (tests/test_penetration_report.py prints them: 1.2e-7 to 4.8e-7 on the spheres, 3.7e-6 on the body's 13 776 faces).  The
integer k and the three flags: equal at every point whose float64 |w| lies within 0.1 of an integer -- on these cases that is every
point.  Bits where the header promises bits.  The tables are integers: equal or not.  Every test prints d, the bound and what the GPU
gave before it asserts.

Shapes: 132 to 200 points over 20 to 384 faces (20 = five trips of four; 20 is no multiple of 16), 1290 points over 2560 faces (two
blocks of 1024 points, the second ragged), 1025 and 1 point, and 3 x 6890 points over the body's 13 776 faces (seven blocks per pose)."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_cases as dc
import penetration_cases as pc
from conftest import PKG_NAME, ROOT

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
F32, F64 = np.float32, np.float64


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _gpu(verts, faces, points):
    """-> wind (B,P) as numpy, status"""
    eng = _mod('engine')
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    w = eng.mesh_winding(T(np.ascontiguousarray(verts, dtype=F32)).to(DEV), T(np.ascontiguousarray(faces, dtype=np.int32)).to(DEV),
                         T(np.ascontiguousarray(points, dtype=F32)).to(DEV), status)
    return w.cpu().numpy(), int(status.item())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(name, w, sl=np.s_[:, :], what=''):
    """wind against the float64 restatement of case `name` within bound(d); k and the three flags exactly where float64 is sure"""
    r64 = pc.reference(name)[sl]
    d = pc.distance(name)
    err = float(np.abs(w.astype(F64) - r64).max())
    print(f'{name}{what} {w.shape}: d {d:.2e} bound {dc.bound(d):.2e} gpu {err:.2e}')
    assert w.shape == r64.shape and err <= dc.bound(d)
    ok = pc.check_cap(name)[sl]
    for got, want in zip(pc.classify(w), pc.classify(r64)):
        assert np.array_equal(got[ok], want[ok])


# ---- 1. against float64 ----
@pytest.mark.parametrize('name', pc.SMALL)
def test_small_meshes_against_float64(name):
    c = pc.small_case(name)
    w, status = _gpu(c['verts'], c['faces'], c['points'])
    assert status == 0
    _check(name, w)


def test_two_spheres_rewound_give_the_same_integers():
    c = pc.small_case('two_spheres')
    w, _ = _gpu(c['verts'], c['faces'], c['points'])
    w2, status = _gpu(c['verts'], c['faces'][:, ::-1].copy(), c['points'])
    d = pc.distance('two_spheres')
    print(f'two_spheres re-wound: | |w| - |w2| | {np.abs(np.abs(w) - np.abs(w2)).max():.2e} bound {dc.bound(d):.2e}')
    assert status == 0 and np.abs(np.abs(w.astype(F64)) - np.abs(w2)).max() <= dc.bound(d) and (np.sign(w) == -np.sign(w2)).all()
    assert np.array_equal(pc.classify(w)[0], pc.classify(w2)[0])
    # through the report: reversed faces turn the normals, the orientation turns the push back
    pr = _mod('penetration_report')
    counts = []
    for faces in (c['faces'], c['faces'][:, ::-1].copy()):
        sign = pr.orientation(c['verts'], faces)
        rep = pr.PenetrationReport(['all'], DEV, faces, 1, 20.0, sign, n_verts=132)
        rep.add(T(c['verts']).to(DEV), None, 0)
        counts.append((sign, rep.finish(reduce=False)['counts'][:, 0].tolist()))
    print('report on both windings (sign, [n_pen, n_thin, n_unsure]):', counts)
    assert counts[0][0] == 1 and counts[1][0] == -1 and counts[0][1] == counts[1][1] and counts[0][1][0] >= 20 and counts[0][1][1] == 0


@pytest.mark.parametrize('P', [1290, 1025, 1])
def test_a_ragged_second_block_of_points(P):
    c = pc.small_case('row')
    w, status = _gpu(c['verts'], c['faces'], c['points'][:, :P])
    assert status == 0
    _check('row', w, np.s_[:, :P], f' P {P}')
    whole, _ = _gpu(c['verts'], c['faces'], c['points'])
    assert np.array_equal(_bits(w), _bits(whole[:, :P]))                      # the same bits in any launch tiling
    tail, _ = _gpu(c['verts'], c['faces'], c['points'][:, 1000:1290])       # columns 1000.. stand in other lanes and another block
    assert np.array_equal(_bits(tail), _bits(whole[:, 1000:1290]))


@pytest.fixture(scope='module')
def body_wind():
    c = pc.body_case()
    w, status = _gpu(c['verts'], c['faces'], c['points'])
    assert status == 0
    return w


def test_body_against_float64(body_wind):
    _check('body', body_wind)
    k, pen, thin, uns = pc.classify(body_wind)
    print('template / bend / moved bend: pen', pen.sum(1).tolist(), 'thin', thin.sum(1).tolist(), 'unsure', uns.sum(1).tolist())
    assert pen[1].sum() >= 300 and pen[0].sum() <= 4 and uns.sum() == 0
    assert np.array_equal(k[1], k[2])                                         # the rigidly moved copy: the same integer at every vertex
    assert (body_wind[0][k[0] == 1] < 0).all()                                # this body is wound inwards


# ---- 2. independence, NaN ----
def test_a_pose_gives_the_same_bits_alone_and_behind_a_nan_pose(body_wind):
    c = pc.body_case()
    alone, _ = _gpu(c['verts'][1:2], c['faces'], c['points'][1:2])
    assert np.array_equal(_bits(alone[0]), _bits(body_wind[1]))
    v = c['verts'].copy()
    v[0, 6889, 2] = np.nan                                                    # the first pose holds a NaN vertex, the middle one is ours
    w, status = _gpu(v, c['faces'], c['points'])
    assert status == 0 and np.isnan(w[0]).all()
    assert np.array_equal(_bits(w[1]), _bits(body_wind[1])) and np.array_equal(_bits(w[2]), _bits(body_wind[2]))


def test_a_nan_point_poisons_itself_only():
    c = pc.small_case('row')
    clean, _ = _gpu(c['verts'], c['faces'], c['points'])
    p = c['points'].copy()
    p[0, 5, 1], p[0, 1024, 0], p[0, 1289, 2] = np.nan, np.inf, -np.inf
    w, status = _gpu(c['verts'], c['faces'], p)
    hit = np.zeros(1290, dtype=bool)
    hit[[5, 1024, 1289]] = True
    assert status == 0 and np.isnan(w[0, hit]).all() and np.array_equal(_bits(w[0, ~hit]), _bits(clean[0, ~hit]))


# ---- 3. defective faces ----
def test_a_face_index_out_of_range_is_skipped_and_reported():
    c = pc.small_case('two_spheres')
    v, f, p = c['verts'], c['faces'], c['points']
    clean, status = _gpu(v, f, p)
    assert status == 0
    for bad in ([0, 1, 132], [-1, 2, 3], [5, 1 << 30, 7]):
        quad = np.concatenate([f, [bad] * 4])                               # four behind the others: every face keeps its partial sum
        w, status = _gpu(v, quad, p)
        assert status == 1 and np.array_equal(_bits(w), _bits(clean)), bad
        w, status = _gpu(v, np.concatenate([f, [bad]]), p)                    # one: the ragged last trip
        assert status == 1 and np.array_equal(_bits(w), _bits(clean)), bad
    w, status = _gpu(v, np.concatenate([[[0, 1, 132]], f]), p)                # in front: the sums are ordered anew
    d = pc.distance('two_spheres')
    print(f'skipped face in front: wind against the mesh without it {np.abs(w - clean).max():.2e}, bound {dc.bound(d):.2e}')
    assert status == 1 and np.abs(w.astype(F64) - pc.reference('two_spheres')).max() <= dc.bound(d)


# ---- 4. arguments ----
def test_batch_zero_and_every_refused_argument():
    eng, lib = _mod('engine'), _mod('_lib').load()
    c = pc.small_case('two_spheres')
    tv, tf, tp = T(c['verts']).to(DEV), T(c['faces']).to(DEV), T(c['points']).to(DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert eng.mesh_winding(tv[:0], tf, tp[:0], status).shape == (0, 132)
    wind = torch.full((1, 132), 7.0, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    none = ctypes.c_void_p(None)
    stream = _mod('_lib').stream_ptr(torch.device(DEV))
    OK, ERR_ARG = 0, lib.jrr_mesh_winding(none, 1, 66, P(tf), 256, P(tp), 132, P(wind), P(status), stream)
    assert ERR_ARG != OK and 'jrr_mesh_winding' in lib.jrr_last_error().decode()
    assert lib.jrr_mesh_winding(P(tv), 0, 132, P(tf), 256, P(tp), 132, P(wind), P(status), stream) == OK          # batch 0: no launch
    args = dict(verts=P(tv), batch=1, n_verts=132, faces=P(tf), n_faces=256, points=P(tp), n_points=132, wind=P(wind), status=P(status))
    for key, value in (('verts', none), ('faces', none), ('points', none), ('wind', none), ('status', none), ('batch', -1), ('n_verts', 0),
                       ('n_verts', 8193), ('n_faces', 0), ('n_points', 0), ('n_points', 65537), ('wind', ctypes.c_void_p(wind.data_ptr() + 2))):
        a = dict(args, **{key: value})
        assert lib.jrr_mesh_winding(*a.values(), stream) == ERR_ARG, key
    acc = torch.zeros(pc.ROW + pc.TRAILER, dtype=torch.int64, device=DEV)
    args = dict(wind=P(wind), part=none, group=none, batch=1, n_verts=132, n_groups=1, acc=P(acc), per_vertex=none, n_pen=none, n_thin=none,
                n_unsure=none)
    assert lib.jrr_penetration_accumulate(*dict(args, batch=0).values(), stream) == OK
    for key, value in (('wind', none), ('acc', none), ('batch', -1), ('n_verts', 0), ('n_verts', 65537), ('n_groups', 0), ('n_groups', 1 << 20),
                       ('acc', ctypes.c_void_p(acc.data_ptr() + 4)), ('n_pen', ctypes.c_void_p(wind.data_ptr() + 2))):
        a = dict(args, **{key: value})
        assert lib.jrr_penetration_accumulate(*a.values(), stream) == ERR_ARG, key
    assert 'jrr_penetration_accumulate' in lib.jrr_last_error().decode()
    torch.cuda.synchronize()
    assert (wind == 7.0).all() and int(acc.abs().sum()) == 0 and int(status.item()) == 0          # no launch wrote anything


# ---- 5. the accumulator ----
def _acc_inputs():
    rs = np.random.RandomState(71)
    B, V = 23, 300
    wind = rs.choice(np.array([0.0, 0.05, 0.5, 0.5000001, 0.93, 1.0, -1.0, 1.07, 1.5, 1.4999999, 1.9, 1.95, -2.0, 2.1, 3.02], dtype=F32), size=(B, V),
                     p=[.05, .02, .01, .01, .03, .5, .25, .03, .01, .01, .02, .02, .02, .01, .01]).astype(F32)
    wind[3] = 1.0                                # a pose without a penetrating vertex
    wind[4, :9], wind[4, 9:] = 2.0, 1.0          # exactly 9, one bit more than 8
    wind[7, 11] = np.nan                         # bad poses
    wind[15, 299] = np.inf
    part = rs.randint(0, 24, size=V).astype(np.int32)
    part[[0, 17]], part[[5, 200]] = -1, 40
    group = (np.arange(B) % 3).astype(np.int32)
    group[[2, 20]] = -1
    group[[9, 22]] = 3
    return wind, part, group


def _run_acc(wind, part, group, n_groups, order=None, splits=None):
    eng = _mod('engine')
    B, V = wind.shape
    acc = torch.zeros(n_groups * pc.ROW + pc.TRAILER, dtype=torch.int64, device=DEV)
    pv = torch.zeros(V, dtype=torch.int64, device=DEV)
    counts = torch.full((3, B), -1, dtype=torch.int32, device=DEV)
    order = np.arange(B) if order is None else order
    tw, tg = T(wind[order]).to(DEV), None if group is None else T(group[order]).to(DEV)
    tp = None if part is None else T(part).to(DEV)
    for a, b in splits or [(0, B)]:
        eng.penetration_accumulate(tw[a:b], tp, None if tg is None else tg[a:b], n_groups, acc, pv, *[counts[k, a:b] for k in range(3)])
    back = np.empty((3, B), dtype=np.int32)
    back[:, order] = counts.cpu().numpy()
    return acc.cpu().numpy(), pv.cpu().numpy(), back


def test_accumulate_word_for_word_in_one_call_and_in_three_in_another_order():
    wind, part, group = _acc_inputs()
    want, want_v, want_c = pc.accumulate(wind, part, group, 3)
    rows = want[:3 * pc.ROW].reshape(3, pc.ROW)
    print('counted', rows[:, pc.COUNT].tolist(), 'bad', rows[:, pc.BAD].tolist(), 'trailer', want[-2:].tolist(), 'pen', rows[:, pc.SUM_PEN].tolist(),
          'thin', rows[:, pc.SUM_THIN].tolist(), 'unsure', rows[:, pc.SUM_UNSURE].tolist(), 'hist', rows[:, pc.HIST:pc.PART].sum(0).tolist())
    assert want[-2:].tolist() == [2, 2] and rows[:, pc.BAD].sum() == 2 and rows[:, pc.COUNT].sum() == 17 and rows[:, pc.PART + 31].sum() > 0
    assert rows[:, pc.HIST].sum() >= 1 and rows[:, pc.HIST + 4].sum() >= 1 and rows[:, pc.SUM_UNSURE].sum() > 0 and rows[:, pc.SUM_THIN].sum() > 0
    one = _run_acc(wind, part, group, 3)
    order = np.random.RandomState(72).permutation(23)
    three = _run_acc(wind, part, group, 3, order, [(0, 5), (5, 6), (6, 23)])
    for got in (one, three):
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want_v) and np.array_equal(got[2], want_c)
    # NULL parts and NULL groups; the counts are optional
    got = _run_acc(wind, None, None, 1)
    w0, v0, c0 = pc.accumulate(wind, None, None, 1)
    assert np.array_equal(got[0], w0) and np.array_equal(got[1], v0) and np.array_equal(got[2], want_c) and w0[pc.PART + 1:pc.PART + 32].sum() == 0
    acc = torch.zeros(3 * pc.ROW + pc.TRAILER, dtype=torch.int64, device=DEV)
    _mod('engine').penetration_accumulate(T(wind).to(DEV), T(part).to(DEV), T(group).to(DEV), 3, acc)
    assert np.array_equal(acc.cpu().numpy(), want)


def test_accumulate_on_the_body(body_wind):
    c = pc.body_case()
    group = np.array([0, 1, 1], dtype=np.int32)
    got = _run_acc(body_wind, c['part'], group, 2)
    want = pc.accumulate(body_wind, c['part'], group, 2)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    ref = pc.accumulate(pc.reference('body').astype(F32), c['part'], group, 2)          # no point is left out: float64 gives the same integers
    assert all(np.array_equal(g, w) for g, w in zip(got, ref))


# ---- 6. the driver ----
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
    """the 6 meshes of penetration_cases.driver_case() as an --eval_vertices directory with two groups; the report without and then
    with --eval_penetration into the same directory"""
    tmp = str(tmp_path_factory.mktemp('penetration'))
    c = pc.driver_case()
    sm = _mod('smpl_model')
    J = sm.default_h36m_regressor()
    ck = os.path.join(tmp, 'retrained_J_Regressor.pt')
    _mod('checkpoint').save_j_regressor(T(J), ck)
    vdir = os.path.join(tmp, 'meshes')
    os.makedirs(vdir)
    np.save(os.path.join(vdir, 'vertices.npy'), c['verts'])
    np.save(os.path.join(vdir, 'gt_j3d.npy'), (J.astype(F64) @ c['verts'].astype(F64) * 1000.0).astype(F32))
    np.save(os.path.join(vdir, 'group.npy'), c['ids'])
    with open(os.path.join(vdir, 'group_names.txt'), 'w') as f:
        f.write('Walking\nSitting\n')
    flags = SYN + ['--batch_size', '4', '--eval_j_regressor', ck, '--eval_vertices', vdir]
    out = os.path.join(tmp, 'one')
    _with_args(flags + ['--eval_report', out], lambda: _mod('eval_report').evaluate_vertices(log=lambda s: None))
    plain = {n: open(os.path.join(out, n), 'rb').read() for n in sorted(os.listdir(out))}
    lines = []
    _with_args(flags + ['--eval_report', out, '--eval_penetration'], lambda: _mod('eval_report').evaluate_vertices(log=lines.append))
    return tmp, flags, out, plain, lines


def test_the_flag_adds_four_files_and_changes_no_other(driver_run):
    tmp, flags, out, plain, lines = driver_run
    now = {n: open(os.path.join(out, n), 'rb').read() for n in sorted(os.listdir(out))}
    assert sorted(set(now) - set(plain)) == ['penetration.json', 'penetration.md', 'penetration.npz', 'penetration_per_vertex.npy']
    for n, data in plain.items():
        assert now[n] == data, n
    assert sum('self-penetration (2 mm push)' in s for s in lines) == 1


def test_the_report_against_the_restatement(driver_run):
    tmp, flags, out, plain, lines = driver_run
    pr = _mod('penetration_report')
    c = pc.driver_case()
    # meshes 0..2 are the body case itself: its float64 reference; 3..5 are rigid copies: the same integers at every vertex
    k, pen, thin, uns = pc.classify(pc.reference('body'))
    src = np.array(c['source'])
    pen, thin, uns = pen[src], thin[src], uns[src]
    doc = pr.load(out)
    assert doc['groups'] == ['Walking', 'Sitting'] and doc['orientation'] == -1 and doc['offset_mm'] == 2.0 and doc['n_verts'] == 6890
    z = np.load(os.path.join(out, 'penetration.npz'))
    print('n_pen', z['n_pen'].tolist(), 'n_thin', z['n_thin'].tolist(), 'n_unsure', z['n_unsure'].tolist())
    assert z['n_pen'].dtype == np.int32 and z['n_pen'].tolist() == pen.sum(1).tolist() and z['n_thin'].tolist() == thin.sum(1).tolist()
    assert z['n_unsure'].tolist() == [0] * 6
    pv = np.load(os.path.join(out, 'penetration_per_vertex.npy'))
    assert pv.dtype == np.int64 and np.array_equal(pv, pen.sum(0))
    want = pr.derive(pc.accumulate(np.where(pen, 2.0, np.where(thin, 0.0, 1.0)).astype(F32), c['part'], c['ids'], 2)[0], pen.sum(0).astype(np.int64),
                     c['names'], c['part'], 24)
    want.pop('per_vertex')
    import json
    assert doc['data'] == json.loads(json.dumps(want))
    r = doc['data']['groups']
    assert r['Walking']['n'] == 3 and r['Sitting']['n'] == 3 and doc['data']['all']['n'] == 6 and doc['data']['all']['n_bad'] == 0
    assert doc['data']['all']['poses_pen8'] == 4 and doc['data']['all']['share_pen8'] == 4 / 6          # the four bends; the template's single vertex is noise
    assert [w['index'] for w in doc['worst']][:4] == [1, 2, 4, 5] and doc['worst'][0]['n_pen'] == int(pen[1].sum())
    assert doc == json.loads(json.dumps(doc))          # load(write(x)) is x
    md = open(os.path.join(out, 'penetration.md')).read()
    a = doc['data']['all']
    assert f'| all | 6 | 0 | {a["poses_pen"]} | {100 * a["share_pen"]:.2f} | 4 | 66.67 | {a["mean_n_pen"]:.2f} |' in md
    assert '| Walking | 3 | 0 |' in md and '| Sitting | 3 | 0 |' in md and 'winding -1 inside' in md
    assert f'| Pelvis | {int((c["part"] == 0).sum())} | {a["per_part"]["Pelvis"]} |' in md and f'| 1 | {int(pen[1].sum())} |' in md


def test_two_gloo_ranks_write_the_same_numbers(driver_run):
    """main.py --eval_vertices --eval_report --eval_penetration under torchrun, two ranks over gloo sharing cuda:0 (3 meshes each): the
    integer tables and the per-mesh counts of disjoint shards sum to those of one rank"""
    tmp, flags, out, plain, lines = driver_run
    pr = _mod('penetration_report')
    out2 = os.path.join(tmp, 'two')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1', '--master-port',
           '29597', os.path.join(ROOT, 'main.py')] + flags + ['--eval_report', out2, '--eval_penetration', '--single_device', '--dist_backend', 'gloo']
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    one, two = pr.load(out), pr.load(out2)
    assert two['data']['all']['n'] == 6 and two['data'] == one['data'] and two['worst'] == one['worst'] and two['per_vertex'] == one['per_vertex']
    assert np.array_equal(np.load(os.path.join(out, 'penetration_per_vertex.npy')), np.load(os.path.join(out2, 'penetration_per_vertex.npy')))
    z1, z2 = np.load(os.path.join(out, 'penetration.npz')), np.load(os.path.join(out2, 'penetration.npz'))
    assert all(np.array_equal(z1[k], z2[k]) for k in ('n_pen', 'n_thin', 'n_unsure'))


def test_each_flag_error_through_the_driver(driver_run):
    tmp, flags, out, plain, lines = driver_run
    run = lambda fl: _with_args(fl, lambda: _mod('eval_report').evaluate_vertices(log=lambda s: None))
    none = os.path.join(tmp, 'none')
    with pytest.raises(ValueError, match='body model'):
        run([f for f in flags if f != '--synthetic'] + ['--eval_report', none, '--eval_penetration'])
    with pytest.raises(ValueError, match='offset_mm'):
        run(flags + ['--eval_report', none, '--eval_penetration', '--eval_penetration_offset_mm', '11'])
    with pytest.raises(ValueError, match='needs --eval_vertices'):
        run(flags + ['--regressor_report', none, '--eval_penetration'])
    assert not os.path.exists(none)
