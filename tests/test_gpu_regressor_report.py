"""The regressor report on the GPU (pytest -m gpu): jrr_regressor_shift_accumulate and jrr_draw_discs against the host restatement
(tests/regressor_report_cases.py), `--regressor_report` through main.py on the synthetic body and through `--eval_vertices`, and two
gloo ranks on one GPU against one.

Bounds.  Tables are integers: equal or not.  Derived means against the float64 restatement on the same float32 inputs: 1e-6 m (the
kernel's float32 arithmetic on values under 0.3 m is about ten roundings of 3e-8 m each); derived standard deviations: 1e-5 m (the
moment words drop up to 2^-32 m^2 per pose: 3e-8 m at the few millimetres of spread these inputs have); the same poses under a rigid
motion: 2e-6 m (the moved inputs are rounded to float32 once more).  Pictures are bytes: equal or not.

Shapes: B = 1, 3, 67, 130 (one thread per pose, 256 per workgroup; 67 and 130 carry the special poses and are split 1 + 66, 64 + 3 and
64 + 66); pictures (1,1), (8,12), (224,224), (224,448) with 1, 3 and 8 sets: one pixel, a picture smaller than a workgroup, several
workgroups per picture, a width that is no multiple of the height."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import regressor_report_cases as rc
from conftest import PKG_NAME, ROOT

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
F32, F64 = np.float32, np.float64


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _acc(n_groups):
    return torch.zeros(n_groups * rc.ROW + rc.TRAILER, dtype=torch.int64, device=DEV)


def _run(ja, jb, group, n_groups=3, pieces=None):
    eng = _mod('engine')
    acc = _acc(n_groups)
    B = ja.shape[0]
    for lo, hi in (pieces or [(0, B)]):
        eng.regressor_shift_accumulate(T(ja[lo:hi]).to(DEV), T(jb[lo:hi]).to(DEV), None if group is None else T(group[lo:hi]).to(DEV),
                                       n_groups, acc)
    return acc.cpu().numpy()


# ---- 1. jrr_regressor_shift_accumulate ----
@pytest.mark.parametrize('B', [1, 3, 67, 130])
def test_shift_table_is_order_free_and_equals_the_restatement(B):
    rr = _mod('regressor_report')
    ja, jb, group = rc.shift_case(B)
    whole = _run(ja, jb, group)
    perm = np.random.RandomState(B).permutation(B)
    assert np.array_equal(_run(ja[perm], jb[perm], group[perm]), whole)
    splits = {1: [], 3: [[(0, 1), (1, 3)]], 67: [[(0, 1), (1, 67)], [(0, 64), (64, 67)]], 130: [[(0, 64), (64, 130)], [(0, 1), (1, 130)]]}[B]
    for pieces in splits:
        assert np.array_equal(_run(ja, jb, group, pieces=pieces), whole), pieces
    want = rc.accumulate(ja, jb, group, 3)
    rows, wrows = whole[:3 * rc.ROW].reshape(3, rc.ROW), want[:3 * rc.ROW].reshape(3, rc.ROW)
    assert np.array_equal(rows[:, rc.COUNT], wrows[:, rc.COUNT]) and np.array_equal(rows[:, rc.BAD], wrows[:, rc.BAD])
    assert np.array_equal(whole[-2:], want[-2:])
    hist = lambda r: r[:, rc.HIST:].reshape(3, 17, 64).sum(-1)
    assert np.array_equal(hist(rows), hist(wrows)) and np.array_equal(hist(rows), np.repeat(rows[:, rc.COUNT, None], 17, 1))
    if B >= 67:
        assert whole[-2] == 2 and whole[-1] == 1 and rows[:, rc.BAD].sum() == 3 and rows[:, rc.COUNT].sum() == B - 6
    differ = int((whole != want).sum())
    print(f'B {B}: {differ} of {whole.size} words differ from the float32 restatement')
    assert differ == 0                              # every operation rounded once, in the header's order: the bits agree
    # the derived numbers against float64
    whole_ok = whole.copy()
    whole_ok[-1] = 0                                # derive refuses a table with ids >= n_groups; the rows are what is measured
    res = rr.derive(whole_ok, ['a', 'b', 'c'])
    for name, keep in [('all', (group >= 0) & (group < 3))] + [(n, group == g) for g, n in enumerate('abc')]:
        r = res['all'] if name == 'all' else res['groups'][name]
        ref = rc.reference_stats(ja, jb, keep)
        assert r['n'] == ref['n']
        if ref['n'] == 0:
            continue
        d_mean = np.abs(np.array(r['mean_mm']) / 1000 - ref['mean']).max()
        d_std = np.abs(np.array(r['std_mm']) / 1000 - ref['std']).max()
        d_abs = max(np.abs(np.array(r['mean_abs_mm']) / 1000 - ref['mean_abs']).max(),
                    np.abs(np.array(r['mean_abs_pelvis_relative_mm']) / 1000 - ref['mean_rel']).max())
        print(f'B {B} {name}: n {r["n"]}  mean {d_mean:.2e} m  std {d_std:.2e} m  lengths {d_abs:.2e} m  (largest |mean| {np.abs(ref["mean"]).max():.3f} m)')
        assert d_mean <= 1e-6 and d_abs <= 1e-6 and d_std <= 1e-5


def test_shift_means_do_not_depend_on_where_the_body_stands():
    rr = _mod('regressor_report')
    ja, jb, group = rc.shift_case(130)
    group = np.where(group == 3, 0, group)
    base = rr.derive(_run(ja, jb, group), ['a', 'b', 'c'])
    ma, mb = rc.moved(ja, jb, seed=77)
    other = rr.derive(_run(ma, mb, group), ['a', 'b', 'c'])
    assert other['all']['n'] == base['all']['n'] == 125 and other['all']['n_bad'] == 3
    for name in ('all', 'a', 'b', 'c'):
        p, q = (r['all'] if name == 'all' else r['groups'][name] for r in (base, other))
        d = np.abs(np.array(p['mean_mm']) - np.array(q['mean_mm'])).max() / 1000
        print(f'{name}: means differ by {d:.2e} m under a rigid motion')
        assert d <= 2e-6


def test_shift_report_add_on_the_device_and_without_groups():
    rr = _mod('regressor_report')
    ja, jb, group = rc.shift_case(67)
    rep = rr.ShiftReport(['only'], DEV)
    rep.add(T(ja[:40]).to(DEV), T(jb[:40]).to(DEV))
    rep.add(T(ja[40:]).to(DEV), T(jb[40:]).to(DEV), None)
    assert np.array_equal(rep.acc.cpu().numpy(), rc.accumulate(ja, jb, None, 1))
    res = rep.finish()
    assert res['all']['n'] == 64 and res['all']['n_bad'] == 3 and res['ignored'] == 0
    with pytest.raises(ValueError, match='int32 tensor on'):
        rep.add(T(ja[:4]).to(DEV), T(jb[:4]).to(DEV), T(group[:4]))
    lib = _mod('_lib')
    with pytest.raises(lib.JrrError, match='n_groups'):
        lib.check(lib.load().jrr_regressor_shift_accumulate(lib.ptr(T(ja).to(DEV)), lib.ptr(T(jb).to(DEV)), None, 67, 0, lib.ptr(rep.acc),
                                                            lib.stream_ptr(torch.device(DEV))), 'shift')


# ---- 2. jrr_draw_discs ----
@pytest.mark.parametrize('n_sets', [1, 3, 8])
@pytest.mark.parametrize('h,w', [(1, 1), (8, 12), (224, 224), (224, 448)])
def test_draw_discs_byte_for_byte(h, w, n_sets):
    eng = _mod('engine')
    rgb, points, radii, colours = rc.disc_case(h, w, n_sets, seed=h + w + n_sets)
    for kind, kw_ref, kw in (('per-point radii', {'radii': radii}, {'radii': T(radii).to(DEV)}), ('scalar radius', {'radius': 2.5}, {'radius': 2.5})):
        pic = T(rgb).to(DEV)
        out = eng.draw_discs(pic, T(points).to(DEV), colours, **kw)
        assert out.data_ptr() == pic.data_ptr()                          # painted INTO the picture
        got, want = out.cpu().numpy(), rc.draw_discs(rgb, points, colours, **kw_ref)
        painted = (want != rgb).any(-1)
        print(f'({h},{w}) {n_sets} sets, {kind}: {int(painted.sum())} of {painted.size} pixels painted, {int((got != want).sum())} bytes differ')
        assert np.array_equal(got, want)
        assert np.array_equal(got[~painted], rgb[~painted])              # every byte outside the discs keeps its value
        if (h, w) != (1, 1):
            assert painted.any()


def test_draw_discs_single_pixels_and_the_later_set_wins():
    eng = _mod('engine')
    pic = torch.zeros(1, 9, 11, 3, dtype=torch.uint8, device=DEV)
    pts = torch.tensor([[[[3.0, 4.0], [20.0, 4.0]]], [[[3.0, 4.0], [7.0, 2.0]]]], device=DEV)      # (2 sets, 1, 2 points, 2)
    out = eng.draw_discs(pic, pts, [(10, 20, 30), (40, 50, 60)], radius=0.0).cpu().numpy()[0]
    assert out[4, 3].tolist() == [40, 50, 60] and out[2, 7].tolist() == [40, 50, 60] and (out.any(-1)).sum() == 2
    half = eng.draw_discs(torch.zeros_like(pic), pts + 0.5, [(1, 1, 1), (2, 2, 2)], radius=0.0)
    assert not half.any()                                                # r = 0 off a pixel centre: nothing


def test_draw_discs_refuses_too_many_sets_or_points_and_touches_nothing():
    eng, lib = _mod('engine'), _mod('_lib')
    pic = torch.full((2, 8, 8, 3), 77, dtype=torch.uint8, device=DEV)
    for n_sets, n_pts in ((9, 4), (2, 257)):
        pts = torch.full((n_sets, 2, n_pts, 2), 3.0, device=DEV)
        with pytest.raises(lib.JrrError, match=r'status -1'):
            eng.draw_discs(pic, pts, [(1, 2, 3)] * n_sets, radius=2.0)
        assert bool((pic == 77).all())
    with pytest.raises(ValueError):
        eng.draw_discs(pic, torch.zeros(1, 3, 4, 2, device=DEV), [(1, 2, 3)])
    with pytest.raises(ValueError):
        eng.draw_discs(pic, torch.zeros(2, 2, 4, 2, device=DEV), [(1, 2, 3)])


# ---- 3. end to end ----
SYN = ['--synthetic', '--device', DEV, '--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent']
SMALL = ['--batch_size', '8', '--synthetic_batches', '2']


def _with_args(flags, fn):
    argsmod = _mod('args')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(flags)
    try:
        return fn()
    finally:
        argsmod._LazyArgs._ns = saved


def _check_files(directory, n_pose, S):
    names = sorted(os.listdir(directory))
    jn = _mod('eval_report').JOINT_NAMES
    assert names == sorted(['regressor.json', 'regressor.md'] + [f'pose_{i:05d}.png' for i in range(n_pose)] +
                           [f'weights_{j:02d}_{jn[j]}.png' for j in range(17)]), names
    for n in names:
        if n.endswith('.png'):
            assert rc.read_png(os.path.join(directory, n)).shape == (S, 2 * S, 3), n


def _check_data(doc, ja, jb, keep_by_group):
    """the data statistics of regressor.json against the float64 restatement on the same joints, within the module's bounds"""
    for name, keep in keep_by_group.items():
        r = doc['data']['all'] if name == 'all' else doc['data']['groups'][name]
        ref = rc.reference_stats(ja, jb, keep)
        assert r['n'] == ref['n'] and r['n_bad'] == 0
        d_mean = np.abs(np.array(r['mean_mm']) / 1000 - ref['mean']).max()
        d_std = np.abs(np.array(r['std_mm']) / 1000 - ref['std']).max()
        d_abs = np.abs(np.array(r['mean_abs_mm']) / 1000 - ref['mean_abs']).max()
        print(f'{doc["source"]} {name}: n {r["n"]}  mean {d_mean:.2e} m  std {d_std:.2e} m  |d| {d_abs:.2e} m')
        assert d_mean <= 1e-6 and d_std <= 1e-5 and d_abs <= 1e-6


def _check_joint_rows(doc, J_a, J_b, v_template):
    rr = _mod('regressor_report')
    A, B = rr.normalised(J_a, np.ones_like(J_a)), rr.normalised(J_b, np.ones_like(J_a))
    for j, r in enumerate(doc['joints']):
        assert r['support_a'] == int((np.maximum(J_a[j], 0) > 0).sum()) and r['support_b'] == int((np.maximum(J_b[j], 0) > 0).sum())
        want = (B[j] - A[j]) @ v_template.astype(F64)
        assert np.abs(np.array(r['template_shift_mm']) / 1000 - want).max() <= 1e-9


@pytest.fixture(scope='module')
def main_run(tmp_path_factory):
    """python main.py --synthetic ... --regressor_report DIR: training (2 batches of 8, 3 inner iterations), then the evaluation"""
    tmp = str(tmp_path_factory.mktemp('regressor_report_main'))
    ck, out = os.path.join(tmp, 'retrained_J_Regressor.pt'), os.path.join(tmp, 'report')
    cmd = [sys.executable, os.path.join(ROOT, 'main.py')] + SYN + SMALL + ['--inner_iters', '3', '--j_step_every', '3', '--no_pose_disc',
                                                                           '--save_j_regressor', ck, '--regressor_report', out]
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return tmp, ck, out, r.stdout


def test_main_writes_the_report_after_training(main_run, smpl_model_np):
    tmp, ck, out, stdout = main_run
    rr, eng, sm = _mod('regressor_report'), _mod('engine'), _mod('smpl_model')
    _check_files(out, 8, 256)
    doc = rr.load(out)
    assert doc['source'] == 'parameters' and doc['groups'] == ['all'] and doc['flags']['batch_size'] == 8
    assert doc['pictures'].startswith('17 weight pictures, 8 pose pictures') and 'regressor report:' in stdout
    assert len(doc['j_regressor_retrained']['sha256_16']) == 16 and doc['data']['all']['n'] == 16 and doc['data']['ignored'] == 0
    # the same joints, recomputed here: the validation batches of test.validation_batches, both regressors on one engine
    J_a = sm.default_h36m_regressor()
    J_b = _mod('checkpoint').load_j_regressor(ck).float().numpy()
    model = sm.synthetic_smpl()
    e = eng.RefineEngine(eng.DeviceModel(model, DEV), 8, flags=eng.FLAG_KEEP_VERTS)
    mask = torch.ones(17, 6890, device=DEV)
    ja, jb = [], []
    for batch in _mod('batches').synthetic_batches(model, J_a, 8, 2, 0 + 7919):
        x6d, betas = batch['pose6d'].to(DEV).float().contiguous(), batch['betas'].to(DEV).float().contiguous()
        for J, dst in ((J_a, ja), (J_b, jb)):
            e.set_j_regressor(T(J).to(DEV), mask)
            dst.append(e.find_joints_forward(betas, x6d=x6d).cpu().numpy())
    ja, jb = np.concatenate(ja), np.concatenate(jb)
    assert not np.array_equal(ja, jb)                                    # training moved the regressor
    _check_data(doc, ja, jb, {'all': np.ones(16, dtype=bool)})
    _check_joint_rows(doc, J_a, J_b, model['v_template'])
    pose = rc.read_png(os.path.join(out, 'pose_00000.png'))
    count = lambda colour: int((pose == np.array(colour, dtype=np.uint8)).all(-1).sum())
    print(f'pose_00000.png: {count(rr.GREEN)} green, {count(rr.BLUE)} blue, {count(rr.RED)} red pixels')
    assert count(rr.RED) >= 17 and count(rr.GREEN) + count(rr.BLUE) > 0  # red is painted last; blue may cover green where the joints coincide


@pytest.fixture(scope='module')
def vertices_run(tmp_path_factory, smpl_model_np):
    """20 meshes of the synthetic body written as an --eval_vertices directory, three groups and one sample marked -1; a retrained
    regressor that differs from the initial one and has lost one support vertex of joint 3 and gained another"""
    tmp = str(tmp_path_factory.mktemp('regressor_report_vertices'))
    eng, sm = _mod('engine'), _mod('smpl_model')
    J = sm.default_h36m_regressor()
    J2 = (J * (1 + 0.5 * np.random.RandomState(5).rand(*J.shape))).astype(F32)
    J2[3, np.flatnonzero(J[3] > 0)[0]] = -1.0
    J2[3, 17] = 0.25
    ck = os.path.join(tmp, 'retrained_J_Regressor.pt')
    _mod('checkpoint').save_j_regressor(T(J2), ck)
    N = 20
    batch = sm.synthetic_batch(smpl_model_np, J, N, seed=123)
    e = eng.RefineEngine(eng.DeviceModel(smpl_model_np, DEV), N, flags=eng.FLAG_KEEP_VERTS)
    e.set_j_regressor(T(J).to(DEV), torch.ones(17, 6890, device=DEV))
    _, verts = e.find_joints_forward(T(batch['betas']).to(DEV), x6d=T(batch['pose6d']).to(DEV), return_verts=True)
    vdir = os.path.join(tmp, 'meshes')
    os.makedirs(vdir)
    np.save(os.path.join(vdir, 'vertices.npy'), verts.cpu().numpy())
    np.save(os.path.join(vdir, 'gt_j3d.npy'), batch['gt_j3d'].astype(F32))
    ids = (np.arange(N) % 3).astype(np.int32)
    ids[4] = -1
    np.save(os.path.join(vdir, 'group.npy'), ids)
    with open(os.path.join(vdir, 'group_names.txt'), 'w') as f:
        f.write('Walking\nSitting\nEating\n')
    flags = SYN + ['--batch_size', '8', '--eval_j_regressor', ck, '--eval_vertices', vdir, '--regressor_report_size', '64',
                   '--regressor_report_images', '5']
    out = os.path.join(tmp, 'one')
    lines = []
    doc = _with_args(flags + ['--regressor_report', out], lambda: _mod('eval_report').evaluate_vertices(log=lines.append))
    return tmp, flags, out, doc, lines, (J, J2, verts, ids)


def test_eval_vertices_writes_the_report_without_the_evaluation_report(vertices_run, smpl_model_np):
    tmp, flags, out, doc, lines, (J, J2, verts, ids) = vertices_run
    rr, eng = _mod('regressor_report'), _mod('engine')
    _check_files(out, 5, 64)                                             # no eval.json: --eval_report was not given
    doc = rr.load(out)
    assert doc['source'] == 'vertices' and doc['groups'] == ['Walking', 'Sitting', 'Eating'] and doc['data']['ignored'] == 1
    assert doc['body_model'].startswith('synthetic') and len(lines) == 1 and lines[0].startswith('regressor report:')
    joints = eng.JointRegressorTable(torch.stack([T(J), T(J2)]).to(DEV), torch.ones(17, 6890, device=DEV)).regress(verts).cpu().numpy()
    keep = {'all': ids >= 0, 'Walking': ids == 0, 'Sitting': ids == 1, 'Eating': ids == 2}
    _check_data(doc, joints[0], joints[1], keep)
    _check_joint_rows(doc, J, J2, smpl_model_np['v_template'])
    assert doc['joints'][3]['shared'] == doc['joints'][3]['support_a'] - 1
    # the raw table is the kernel's on these joints
    want = rc.accumulate(joints[0], joints[1], ids, 3)
    assert [doc['data']['groups'][n]['raw'] for n in doc['groups']] == want[:3 * rc.ROW].reshape(3, rc.ROW).tolist()


def test_weight_pictures_are_the_restatements_discs_on_the_shaded_template(vertices_run, smpl_model_np):
    tmp, flags, out, doc, lines, (J, J2, verts, ids) = vertices_run
    rr, eng = _mod('regressor_report'), _mod('engine')
    pics = rr.Pictures(smpl_model_np, eng.DeviceModel(smpl_model_np, DEV), 64)
    front, side, fxy, sxy, rad, colours = pics.weight_layers(J, J2, np.ones_like(J))
    assert front.shape == (17, 64, 64, 3) and fxy.shape[:2] == (4, 17) and rad.shape == fxy.shape[:3]
    want = np.concatenate([rc.draw_discs(front.cpu().numpy(), fxy.cpu().numpy(), colours, radii=rad.cpu().numpy()),
                           rc.draw_discs(side.cpu().numpy(), sxy.cpu().numpy(), colours, radii=rad.cpu().numpy())], axis=2)
    jn = _mod('eval_report').JOINT_NAMES
    green, blue = np.array(rr.GREEN, dtype=np.uint8), np.array(rr.BLUE, dtype=np.uint8)
    for j in range(17):
        got = rc.read_png(os.path.join(out, f'weights_{j:02d}_{jn[j]}.png'))
        assert np.array_equal(got, want[j]), j
    is_green, is_blue = (want[3] == green).all(-1), (want[3] == blue).all(-1)
    got = rc.read_png(os.path.join(out, f'weights_03_{jn[3]}.png'))
    assert is_green.any() and is_blue.any()                              # joint 3 lost a vertex (green alone) and gained one (blue alone)
    assert np.array_equal((got == green).all(-1), is_green) and np.array_equal((got == blue).all(-1), is_blue)
    # the projected support vertices lie on the body's picture, and the discs have the stated radii
    r = rad.cpu().numpy()
    A = rr.normalised(J, np.ones_like(J))
    assert np.allclose(np.sort(r[0, 3][np.isfinite(r[0, 3])]), np.sort(1.5 + 6 * np.sqrt(A[3][A[3] > 0])), atol=1e-6)
    assert r[2, 3, 0] == 4.0 and np.isnan(r[2, 3, 1:]).all()
    xy = fxy.cpu().numpy()[0, 3]
    assert np.nanmin(xy) >= -0.5 and np.nanmax(xy) <= 63.5


def test_without_a_body_model_the_numbers_are_written_alone(vertices_run):
    tmp, flags, out, doc, lines, _ = vertices_run
    rr = _mod('regressor_report')
    no_synth = [f for f in flags if f != '--synthetic'] + ['--j_regressor_init', 'SPIN/data/J_regressor_h36m.npy']
    out2 = os.path.join(tmp, 'numbers')
    said = []
    with pytest.warns(RuntimeWarning):                                   # the default initial regressor path falls back to the shipped support
        _with_args(no_synth + ['--regressor_report', out2], lambda: _mod('eval_report').evaluate_vertices(log=said.append))
    assert sorted(os.listdir(out2)) == ['regressor.json', 'regressor.md']
    doc2 = rr.load(out2)
    assert doc2['pictures'] == 'skipped: no body model' and doc2['data'] == rr.load(out)['data']
    assert all(r['template_shift_mm'] is None for r in doc2['joints'])
    assert len(said) == 2 and 'no body model' in said[0]


def test_two_gloo_ranks_equal_one_rank(vertices_run):
    """main.py --eval_vertices --regressor_report under torchrun, two ranks over gloo sharing cuda:0 (10 meshes each, chunks of 8 + 2)"""
    tmp, flags, out, doc, lines, _ = vertices_run
    rr = _mod('regressor_report')
    out2 = os.path.join(tmp, 'two')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1', '--master-port',
           '29587', os.path.join(ROOT, 'main.py')] + flags + ['--regressor_report', out2, '--single_device', '--dist_backend', 'gloo']
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    one, two = rr.load(out), rr.load(out2)
    _check_files(out2, 5, 64)
    assert two['data']['all']['n'] == 19 and two['data'] == one['data'] and two['joints'] == one['joints']
