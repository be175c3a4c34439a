"""`--place_refined` without a GPU: the float64 restatement (tests/place_cases.py) against itself and first principles, the row layout
of the C ABI against its Python mirrors, the refined_placed.npz / place.json / meta.json files through refined.place with the two
operators replaced by the restatement, the row-count errors of the command, and the flags."""
import importlib
import json
import os
import pickle
import re

import numpy as np
import pytest
import torch

import place_cases as pc
import refined_cases as rc
from conftest import PKG_NAME, ROOT

F, F64 = np.float32, np.float64
T = torch.from_numpy


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


@pytest.fixture(scope='module')
def regular():
    joints, j2d, K, weight, planted, exact = pc.regular_cases(200, seed=0)
    return dict(joints=joints, j2d=j2d, K=K, weight=weight, planted=planted, exact=exact, res=pc.place(joints, j2d, K, weight, 10))


# ---- 1. the restatement ----
def test_the_case_set_is_what_the_docstring_says(regular):
    K, w = regular['K'], regular['weight']
    assert (K[:, 0, 0] != K[:, 1, 1]).all() and K[:, [0, 1], [0, 1]].min() >= 1100 and K[:, [0, 1], [0, 1]].max() <= 1200
    assert K[:, :2, 2].min() >= 480 and K[:, :2, 2].max() <= 540
    t = regular['planted']
    assert t[:, 2].min() >= 2.5 and t[:, 2].max() <= 7 and np.abs(t[:, :2]).max() <= 1.5 and np.abs(t[:, :2]).max() > 1.2
    assert regular['exact'].sum() == 100
    zeroed = (w == 0).sum(1)
    assert set(zeroed.tolist()) == {0, 5} and (zeroed == 5).sum() == 66 and ((w != 1) & (w != 0)).any(1).sum() == 40
    exact_uv = pc.project64(regular['joints'], t, K)[0]
    assert np.array_equal(regular['j2d'][regular['exact']], exact_uv[regular['exact']].astype(F))
    noise = (regular['j2d'] - exact_uv)[~regular['exact']]
    assert 4.5 < noise.std() < 5.5


def test_every_refusal_bit_is_reported_and_none_on_the_regular_cases(regular):
    assert (regular['res']['status'] == 0).all() and np.isfinite(regular['res']['trans']).all()
    seen = 0
    for name, bit in pc.REFUSALS.items():
        r = pc.place(*(a[None] for a in pc.refusal_case(name)), n_iters=10)
        assert r['status'].tolist() == [bit], name
        assert np.isnan(r['trans']).all() and np.isnan(r['trans_linear']).all() and np.isnan(r['err']).all() and np.isnan(r['err_lin']).all()
        seen |= bit
    assert seen == pc.BAD_BITS
    joints, j2d, K, weight, planted, reg = pc.gpu_pool()
    r = pc.place(joints, j2d, K, weight, 1)
    assert (r['status'][reg] == 0).all() and (r['status'][~reg] != 0).all() and (~reg).sum() == 8 and reg[0]


def test_exact_pixels_recover_the_planted_translation(regular):
    d = np.abs(regular['res']['trans'] - regular['planted']).max(1)
    print(f'exact pixels: {d[regular["exact"]].max():.3e} m; noisy pixels: {d[~regular["exact"]].max():.3e} m')
    assert d[regular['exact']].max() <= 1e-5
    assert np.abs(regular['res']['trans_linear'] - regular['planted']).max(1)[regular['exact']].max() <= 1e-5
    assert d[~regular['exact']].max() > 1e-3                                           # 5 px of noise do move the body


def _gradient(case, t, h=1e-5):
    g = np.zeros_like(t)
    for c in range(3):
        e = np.zeros(3)
        e[c] = h
        g[:, c] = (pc.cost64(case['joints'], case['j2d'], case['K'], case['weight'], t + e) -
                   pc.cost64(case['joints'], case['j2d'], case['K'], case['weight'], t - e)) / (2 * h)
    return np.linalg.norm(g, axis=1)


def test_the_result_of_the_noisy_cases_is_a_stationary_point(regular):
    noisy = ~regular['exact']
    ratio = _gradient(regular, regular['res']['trans'])[noisy] / _gradient(regular, regular['res']['trans_linear'])[noisy]
    print(f'|gradient| at the result / at the linear start: max {ratio.max():.3e}, median {np.median(ratio):.3e}')
    assert ratio.max() <= 1e-6


def test_the_cost_never_rises_and_forty_more_steps_change_nothing(regular):
    costs, accepted = regular['res']['costs'], regular['res']['accepted']
    assert costs.shape == (11, 200) and (np.diff(costs, axis=0) <= 0).all()
    assert np.array_equal(np.diff(costs, axis=0) < 0, accepted) and accepted[0].all() and not accepted[-1].all()
    np.testing.assert_allclose(costs[0], pc.cost64(regular['joints'], regular['j2d'], regular['K'], regular['weight'], regular['res']['trans_linear']), rtol=1e-12)
    np.testing.assert_allclose(costs[-1], pc.cost64(regular['joints'], regular['j2d'], regular['K'], regular['weight'], regular['res']['trans']), rtol=1e-12)
    more = pc.place(regular['joints'], regular['j2d'], regular['K'], regular['weight'], 50)
    d = np.abs(more['trans'] - regular['res']['trans']).max()
    print(f'10 -> 50 steps: {d:.3e} m')
    assert d <= 1e-9
    zero = pc.place(regular['joints'], regular['j2d'], regular['K'], regular['weight'], 0)
    assert np.array_equal(zero['trans'], zero['trans_linear']) and np.array_equal(zero['err'], zero['err_lin'])
    assert np.array_equal(zero['trans'], regular['res']['trans_linear'])


def test_weight_zero_joints_do_not_move_the_result(regular):
    joints, j2d, w = regular['joints'].copy(), regular['j2d'].copy(), regular['weight']
    dropped = w == 0
    joints[dropped] += F(0.3)
    j2d[dropped] -= F(200.0)
    r = pc.place(joints, j2d, regular['K'], w, 10)
    assert np.array_equal(r['trans'], regular['res']['trans']) and np.array_equal(r['status'], regular['res']['status'])
    assert np.array_equal(r['err'][~dropped], regular['res']['err'][~dropped]) and not np.array_equal(r['err'][dropped], regular['res']['err'][dropped])
    # weights None are ones; a common factor on the weights leaves the minimiser where it is
    ones = pc.place(regular['joints'], regular['j2d'], regular['K'], np.ones_like(w), 10)
    none = pc.place(regular['joints'], regular['j2d'], regular['K'], None, 10)
    assert np.array_equal(ones['trans'], none['trans']) and np.isfinite(none['trans']).all()
    scaled = pc.place(regular['joints'], regular['j2d'], regular['K'], 4 * w, 10)
    assert np.abs(scaled['trans'] - regular['res']['trans']).max() <= 1e-9


def test_projection_reference_and_table_restatement():
    for N in pc.PROJECT_POINTS:
        points, trans, K = pc.project_case(N)
        uv, depth, bound = pc.project_reference(points, trans, K)
        behind = np.isnan(uv[..., 0])
        assert behind.any() and not behind.all() and np.array_equal(behind, ~(depth > 0)) and behind[1, 0] and (N == 1 or depth[1, 0] == 0.0)
        assert (bound[~behind] > 0).all() and np.median(bound[~behind]) < 2e-3
    assert pc.fixed24(F([1.0, 0.5, 2.0 ** -24, 999.0])).tolist() == [1 << 24, 1 << 23, 1, 999 << 24]
    trans = np.array([[0, 0, 4.0], [0, 0, 5.0], [0, 0, np.nan], [0, 0, 3.0]])
    err = np.full((4, 17), 2.0, F)
    err[3, 5] = 2000.0
    w = np.ones((4, 17), F)
    w[0, :3] = 0
    t = pc.accumulate(trans, err / 2, err, w, np.array([0, 8, 1, 0], np.int32), np.array([0, 0, 0, 0], np.int32), 1)
    assert t[pc.COUNT] == 2 and t[pc.BAD] == 2 and t[pc.STEP_PIVOT] == 1 and t[pc.SUM_TZ] == 9 << 24
    assert t[pc.JOINTS:pc.JOINTS + 17].tolist() == [1] * 3 + [2] * 14 and t[pc.SUM_ERR + 4] == 4 << 24 and t[pc.SUM_ERR_LIN] == 1 << 24
    doc = _mod('place_report').derive(t, ['all'])
    a = doc['all']
    assert a['n'] == 2 and a['n_bad'] == 2 and a['n_step_pivot'] == 1 and a['depth_m'] == 4.5 and a['reproj_px'] == 2.0 and a['reproj_linear_px'] == 1.0
    assert a['reproj_per_joint_px'] == [2.0] * 17 and a['joints_n'][0] == 1
    empty = _mod('place_report').derive(np.zeros(57, np.int64), ['all'])['all']
    assert empty['depth_m'] is None and empty['reproj_px'] is None and empty['reproj_per_joint_px'] == [None] * 17


# ---- 2. the C ABI ----
def test_row_layout_is_stated_once_and_mirrored():
    hdr = open(os.path.join(ROOT, 'include', 'jrr.h')).read()
    enum = {k: int(v) for k, v in re.findall(r'\b(JRR_PLACE_[A-Z0-9_]+) = (\d+)', hdr)}
    pr, eng, refined = _mod('place_report'), _mod('engine'), _mod('refined')
    for mirror in (pr, pc):
        assert (mirror.ROW, mirror.TRAILER, mirror.COUNT, mirror.BAD, mirror.STEP_PIVOT, mirror.SUM_TZ, mirror.JOINTS, mirror.SUM_ERR_LIN, mirror.SUM_ERR) == \
            tuple(enum['JRR_PLACE_ACC_' + k] for k in ('ROW', 'TRAILER', 'COUNT', 'BAD', 'STEP_PIVOT', 'SUM_TZ', 'JOINTS', 'SUM_ERR_LIN', 'SUM_ERR'))
        assert mirror.BAD_BITS == enum['JRR_PLACE_BAD_BITS']
    assert pr.LAYOUT_VERSION == enum['JRR_PLACE_ACC_LAYOUT_VERSION'] and sorted(pr.STATUS_BITS) == [1, 2, 4, 8]
    assert (pc.BIT_FEW, pc.BIT_PIVOT, pc.BIT_BEHIND, pc.BIT_STEP) == (enum['JRR_PLACE_FEW_OR_NONFINITE'], enum['JRR_PLACE_LINEAR_PIVOT'],
                                                                      enum['JRR_PLACE_LINEAR_BEHIND'], enum['JRR_PLACE_STEP_PIVOT'])
    assert (eng.PLACE_ACC_ROW, eng.PLACE_ACC_TRAILER, eng.PLACE_MAX_ITERS) == (enum['JRR_PLACE_ACC_ROW'], enum['JRR_PLACE_ACC_TRAILER'], enum['JRR_PLACE_MAX_ITERS'])
    assert refined.PLACE_MAX_ITERS == enum['JRR_PLACE_MAX_ITERS'] and refined.PLACE_NAME == 'refined_placed.npz'
    sig = _mod('_lib').SIGNATURES
    assert len(sig['jrr_place_translation'][1]) == 11 and len(sig['jrr_project_points'][1]) == 8 and len(sig['jrr_place_accumulate'][1]) == 10
    src = open(os.path.join(ROOT, PKG_NAME, 'csrc', 'place.hip')).read()
    assert 'place.hip' in _mod('build').SOURCES and 'atomicAdd(' not in src and 'float atomic' not in src      # integer atomics through acctab.h only


# ---- 3. the files, with the operators restated on the host ----
N_ROWS = 30


def _host_operators(monkeypatch):
    """engine.place_translation / place_accumulate on CPU tensors by the restatement (the GPU tests hold the kernels to it)"""
    engine = _mod('engine')

    def place_translation(joints, j2d, K, weight=None, n_iters=10, out=None):
        r = pc.place(joints.numpy(), j2d.numpy(), K.numpy(), None if weight is None else weight.numpy(), n_iters)
        trans, err_lin, err, status = out
        trans.copy_(T(r['trans'])); err.copy_(T(r['err'])); status.copy_(T(r['status']))
        if err_lin is not None:
            err_lin.copy_(T(r['err_lin']))
        return out

    def place_accumulate(trans, err_lin, err, weight, status, group, n_groups, acc):
        acc += T(pc.accumulate(trans.numpy(), err_lin.numpy(), err.numpy(), None if weight is None else weight.numpy(), status.numpy(),
                               None if group is None else group.numpy(), n_groups))

    for f in (place_translation, place_accumulate):
        monkeypatch.setattr(engine, f.__name__, f)


def _write_table(directory, seed=4):
    """DIR/refined.npz + meta.json of 30 rows, 24 of them refined; the per-row `joints` the stand-in joints_of returns; intrinsics and
    full-frame pixels made from planted translations (rows 3 and 18: a NaN pixel, a body behind the camera)"""
    refined = _mod('refined')
    rng = np.random.RandomState(seed)
    x6d, betas, cam = rng.normal(size=(N_ROWS, 24, 6)).astype(F), rng.normal(size=(N_ROWS, 10)).astype(F), rng.normal(size=(N_ROWS, 3)).astype(F)
    table = rc.host_rows(x6d, betas, cam, rng.uniform(size=(N_ROWS, 7)).astype(F))
    unrefined = np.arange(N_ROWS) % 5 == 2
    table[unrefined] = 0
    t = refined.RefinedTable(N_ROWS, 'cpu')
    t.table.copy_(T(table))
    raw = t.finish(directory, {'inner_iters': 3, 'data': 'dataset'})
    joints, K = pc.bodies(N_ROWS, rng), pc.cameras(N_ROWS, rng)
    planted = np.stack([rng.uniform(-1.5, 1.5, N_ROWS), rng.uniform(-1.5, 1.5, N_ROWS), rng.uniform(2.5, 7.0, N_ROWS)], 1)
    planted[18, 2] = -5.0
    j2d = (pc.project64(joints, planted, K)[0] + rng.normal(0, 2.0, size=(N_ROWS, 17, 2))).astype(F)
    j2d[3, 4, 0] = np.nan
    paths = [f'/data/h36m/S{9 + 2 * (i % 2)}/{"Walking 1" if i < 16 else "Eating 2"}/imageSequence/1/img_{i + 1:06d}.jpg' for i in range(N_ROWS)]
    return raw, joints, K, j2d, planted, paths, unrefined


def _joints_of(joints):
    fn = lambda arrays, rows: T(joints[rows])
    fn.name = 'stand-in regressor'
    return fn


def test_place_files_round_trip_through_load(tmp_path, monkeypatch):
    refined, pr = _mod('refined'), _mod('place_report')
    _host_operators(monkeypatch)
    out_dir = str(tmp_path / 'ref')
    raw, joints, K, j2d, planted, paths, unrefined = _write_table(out_dir)
    raw_bytes = open(os.path.join(out_dir, 'refined.npz'), 'rb').read()
    meta_before = json.load(open(os.path.join(out_dir, 'meta.json')))
    weights = np.ones((N_ROWS, 17), F)
    weights[5, :4] = 0
    out = refined.place(out_dir, K, j2d, paths, _joints_of(joints), n_iters=10, weights=weights, weights_name='w.npy', batch_size=7, device='cpu')
    assert sorted(os.listdir(out_dir)) == ['meta.json', 'place.json', 'place.md', 'refined.npz', 'refined_placed.npz']
    assert open(os.path.join(out_dir, 'refined.npz'), 'rb').read() == raw_bytes          # refined.npz itself is not rewritten
    back = refined.load(out_dir, n=N_ROWS, name=refined.PLACE_NAME)
    meta = back.pop('meta')
    new = {'trans', 'trans_linear', 'reproj_px', 'reproj_px_linear', 'place_status'}
    assert set(back) == (set(raw) - {'meta'}) | new
    assert all(np.array_equal(back[k], raw[k], equal_nan=True) for k in raw if k != 'meta')      # every array of the input, unchanged
    assert all(np.array_equal(back[k], out[k], equal_nan=True) for k in back)
    assert back['trans'].dtype == F64 and back['trans'].shape == (N_ROWS, 3) and back['trans_linear'].dtype == F64
    assert back['reproj_px'].dtype == F and back['reproj_px'].shape == (N_ROWS, 17) and back['reproj_px_linear'].dtype == F
    assert back['place_status'].dtype == np.int32 and back['place_status'].shape == (N_ROWS,)
    # rows without a refined pose: NaN and -1; the refused rows: NaN and their bit; the rest: the restatement's, chunk by chunk
    assert (back['place_status'][unrefined] == -1).all() and np.isnan(back['trans'][unrefined]).all() and np.isnan(back['reproj_px'][unrefined]).all()
    rows = np.nonzero(~unrefined)[0]
    want = pc.place(joints[rows], j2d[rows], K[rows], weights[rows], 10)
    assert np.array_equal(back['trans'][rows], want['trans'], equal_nan=True) and np.array_equal(back['trans_linear'][rows], want['trans_linear'], equal_nan=True)
    assert np.array_equal(back['reproj_px'][rows], want['err'], equal_nan=True) and np.array_equal(back['reproj_px_linear'][rows], want['err_lin'], equal_nan=True)
    assert back['place_status'][3] == pc.BIT_FEW and back['place_status'][18] == pc.BIT_BEHIND and np.isnan(back['trans'][[3, 18]]).all()
    good = rows[(want['status'] == 0)]
    assert good.size == 22 and np.abs(back['trans'][good] - planted[good]).max() < 0.2
    # the report
    doc = pr.load(out_dir)
    assert doc['groups'] == ['Eating', 'Walking'] and doc['group_kind'] == 'action' and doc['n_iters'] == 10 and doc['j_regressor'] == 'stand-in regressor'
    assert doc['weights'] == 'w.npy' and doc['status_counts'] == {'1': 1, '2': 0, '4': 1, '8': 0} and doc['root_err'] is False
    a = doc['table']['all']
    assert a['n'] == 22 and a['n_bad'] == 2 and doc['table']['groups']['Walking']['n'] + doc['table']['groups']['Eating']['n'] == 22
    assert a['joints_n'] == [21] * 4 + [22] * 13 and 'root_err_mm' not in a
    np.testing.assert_allclose(a['depth_m'], back['trans'][good, 2].mean(), rtol=1e-6)
    part = weights[good] > 0
    np.testing.assert_allclose(a['reproj_px'], back['reproj_px'][good][part].astype(F64).mean(), rtol=1e-6)
    assert a['reproj_px'] < a['reproj_linear_px']
    per_pose = np.array([back['reproj_px'][i][weights[i] > 0].astype(F64).mean() for i in good])
    assert doc['pose_error_px'] == {'n': 22, 'median': float(np.median(per_pose)), 'p95': float(np.percentile(per_pose, 95))}
    md = open(os.path.join(out_dir, 'place.md'), encoding='utf-8').read()
    assert '| Walking |' in md and '| R_Wrist |' in md and md.rstrip().endswith(pr.summary_line(doc)) and 'pelvis' not in md
    assert {k: v for k, v in meta.items() if k != 'place'} == meta_before and meta['place']['placed'] == 22 and meta['place']['rows'] == 24
    assert meta['place']['source'] == 'refined.npz'
    # a camera-frame ground truth: the distance of the placed pelvis from the measured one; and a named .npz as the input
    gt = ((joints + planted[:, None]) * 1000).astype(F)
    out2 = refined.place(os.path.join(out_dir, refined.PLACE_NAME), K, j2d, None, _joints_of(joints), n_iters=3, gt_j3d_mm=gt, group_kind='none', device='cpu')
    doc2 = pr.load(out_dir)
    assert doc2['root_err'] is True and doc2['groups'] == ['all'] and doc2['n_iters'] == 3 and doc2['weights'] is None
    want_root = np.linalg.norm(out2['trans'][good] - planted[good], axis=1).mean() * 1000
    np.testing.assert_allclose(doc2['table']['all']['root_err_mm'], want_root, rtol=1e-3)
    assert 'pelvis' in open(os.path.join(out_dir, 'place.md'), encoding='utf-8').read() and out2['meta']['place']['source'] == refined.PLACE_NAME
    assert np.array_equal(out2['pose6d'], raw['pose6d'])
    # the placed file reads as the smoothed one does
    by_file = refined.load_path(os.path.join(out_dir, refined.PLACE_NAME), n=N_ROWS)
    assert 'trans' in by_file and np.array_equal(by_file['pose6d'], raw['pose6d'])
    for bad, message in ((dict(intrinsics=K[:-1]), 'intrinsics should be'), (dict(gt_j2d=j2d[:, :16]), 'gt_j2d should be'),
                         (dict(weights=weights[:, :5]), 'weights should be'), (dict(n_iters=65), 'n_iters 65: 0 .. 64'), (dict(paths=paths[:-1]), '29 paths')):
        kw = dict(dict(intrinsics=K, gt_j2d=j2d, paths=paths), **bad)
        with pytest.raises(ValueError, match=message):
            refined.place(out_dir, kw.pop('intrinsics'), kw.pop('gt_j2d'), kw.pop('paths'), _joints_of(joints), device='cpu', **kw)


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


def test_command_refuses_a_split_of_another_length_and_flags_default_to_off(tmp_path, monkeypatch):
    a, refined = _mod('args'), _mod('refined')
    ns = a.get_args([])
    assert ns.place_refined is None and ns.place_iters == 10 and ns.place_weights is None
    ns = a.get_args(['--place_refined', 'dir/refined_fused.npz', '--place_iters', '4', '--place_weights', 'w.npy'])
    assert ns.place_refined == 'dir/refined_fused.npz' and ns.place_iters == 4 and ns.place_weights == 'w.npy'
    for k, v in a.REFERENCE_FLAGS.items():
        assert getattr(ns, k) == v, k
    # the flags of the command appear in no record of flags that another command writes
    recorded = a.recorded(ns)
    assert set(vars(ns)) - set(vars(recorded)) == {'place_refined', 'place_iters', 'place_weights'} == set(a.PLACE_FLAGS)
    assert a.recorded(vars(ns)) == vars(recorded) and _mod('regressor_fit').flags_doc(ns) == _mod('regressor_fit').flags_doc(a.get_args([]))
    for name in ('test.py', 'eval_report.py', 'regressor_report.py', 'regressor_fit.py', 'refined.py'):      # every record of flags passes through it
        assert 'flags_doc(jargs.recorded(' in open(os.path.join(ROOT, PKG_NAME, name)).read(), name
    assert 'place_command()' in open(os.path.join(ROOT, 'main.py')).read()
    _host_operators(monkeypatch)
    out_dir = str(tmp_path / 'ref')
    _write_table(out_dir)
    root = str(tmp_path / 'data')
    os.makedirs(root)
    _write_split(root, N_ROWS - 1)
    saved = a._LazyArgs._ns
    try:
        a._LazyArgs._ns = a.get_args(['--place_refined', out_dir])
        with pytest.raises(ValueError, match='--place_refined needs --data_root'):
            refined.place_command(log=lambda s: None)
        a._LazyArgs._ns = a.get_args(['--place_refined', out_dir, '--data_root', root, '--place_iters', '65'])
        with pytest.raises(ValueError, match='--place_iters 65: 0 .. 64'):
            refined.place_command(log=lambda s: None)
        a._LazyArgs._ns = a.get_args(['--place_refined', out_dir, '--data_root', root])
        with pytest.raises(FileNotFoundError, match='images.pkl'):
            refined.place_command(log=lambda s: None)
        with open(os.path.join(root, 'precomputed_val', 'images.pkl'), 'wb') as f:
            pickle.dump([f'/data/S9/Walking/imageSequence/1/img_{k:06d}.jpg' for k in range(N_ROWS - 1)], f)
        with pytest.raises(ValueError, match='the table holds 30 samples, the split 29 with 29 frame paths'):
            refined.place_command(log=lambda s: None)
        os.environ['RANK'] = '1'                                                          # one process: another rank returns at once
        try:
            assert refined.place_command(log=lambda s: None) is None
        finally:
            del os.environ['RANK']
    finally:
        a._LazyArgs._ns = saved
    assert sorted(os.listdir(out_dir)) == ['meta.json', 'refined.npz']


def test_dump_eval_vertices_placed_needs_the_table():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'dump_eval_vertices.py'), 'nowhere', '--placed'], capture_output=True, text=True)
    assert r.returncode != 0 and '--placed needs --gt_refined' in r.stderr
