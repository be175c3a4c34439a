"""The regressor report on the CPU: known answers of the host restatement (tests/regressor_report_cases.py) that the GPU tests measure
against, `derive` on hand-built tables, the flags, report.frame_camera, compare_regressors, and the evaluation driver's engine calls
with and without `--regressor_report` under a recording fake."""
import importlib
import os

import numpy as np
import pytest
import torch

import regressor_report_cases as rc
from conftest import PKG_NAME

F32, F64 = np.float32, np.float64


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _with_args(flags, fn):
    argsmod = _mod('args')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(list(flags))
    try:
        return fn()
    finally:
        argsmod._LazyArgs._ns = saved


# ---- 1. the restatement's own known answers ----
def test_layout_constants_agree_with_the_header_and_the_module():
    from conftest import ROOT
    rr, eng = _mod('regressor_report'), _mod('engine')
    hdr = open(os.path.join(ROOT, 'include', 'jrr.h')).read()
    import re
    val = lambda name: int(re.search(rf'\b{name} = (\d+)', hdr).group(1))
    for mod in (rc, rr):
        assert (mod.ROW, mod.COUNT, mod.BAD, mod.SUM, mod.MOM, mod.ABS, mod.ABS_REL, mod.HIST, mod.BINS, mod.TRAILER) == tuple(
            val('JRR_SHIFT_ACC_' + k) for k in ('ROW', 'COUNT', 'BAD', 'SUM', 'MOM', 'ABS', 'ABS_REL', 'HIST', 'BINS', 'TRAILER'))
    assert rr.LAYOUT_VERSION == val('JRR_SHIFT_ACC_LAYOUT_VERSION')
    assert (eng.SHIFT_ACC_ROW, eng.SHIFT_ACC_TRAILER) == (rc.ROW, rc.TRAILER)
    assert (eng.DISCS_MAX_SETS, eng.DISCS_MAX_POINTS) == (val('JRR_DISCS_MAX_SETS'), val('JRR_DISCS_MAX_POINTS'))
    assert rc.HIST + rc.NJ * rc.BINS == rc.ROW and rc.MOM == rc.SUM + 51 and rc.ABS == rc.MOM + 102


@pytest.mark.parametrize('dtype', [F32, F64])
def test_upright_skeleton_gives_the_identity_frame(dtype):
    a = rc.UPRIGHT[None].astype(F32)
    t = rc.shift_terms(a, a, dtype)
    assert np.array_equal(t['frame'][0], np.eye(3)) and t['good'][0] and not t['c'].any()


@pytest.mark.parametrize('t_up', [0.0131, 0.0511, 0.1255])
def test_a_shift_along_the_bodys_up_axis_under_random_rigid_motions(t_up):
    """B = A + t * (body up): mean (0, t, 0), no spread beyond the moment words' resolution, the median in the bin of t"""
    rr = _mod('regressor_report')
    rs = np.random.RandomState(3)
    n = 40
    R, shift = rc.rotations(n, rs), rs.randn(n, 3) * 0.4
    A = np.einsum('brc,jc->bjr', R, rc.UPRIGHT) + shift[:, None]
    Bj = A + t_up * R[:, None, :, 1]
    ja, jb = A.astype(F32), Bj.astype(F32)
    t64 = rc.shift_terms(ja, jb, F64)
    assert t64['good'].all() and np.abs(t64['c'] - [0, t_up, 0]).max() <= 3e-7           # float32 inputs of ~1 m: 6e-8 each
    res = rr.derive(rc.accumulate(ja, jb, None, 1), ['all'])['all']
    assert res['n'] == n and res['n_bad'] == 0
    assert np.abs(np.array(res['mean_mm']) - [0, t_up * 1000, 0]).max() <= 1e-3          # 1e-6 m
    # a moment word drops up to 2^-32 m^2 per pose: a standard deviation below sqrt(2^-32) m = 0.015 mm cannot be told from zero
    assert np.array(res['std_mm']).max() <= 0.02
    assert np.abs(np.array(res['mean_abs_mm']) - t_up * 1000).max() <= 1e-3
    assert np.abs(np.array(res['mean_abs_pelvis_relative_mm'])).max() <= 1e-3
    want_bin = int(np.floor(t_up * 500))
    assert res['median_abs_mm'] == [(want_bin + 1) * 2.0] * 17 and res['p95_abs_mm'] == res['median_abs_mm']


def test_degenerate_and_non_finite_poses_land_in_bad_only():
    ja, jb, _ = rc.shift_case(6, seed=8)
    jb[0, 2, 1] = np.nan
    ja[1, 16, 0] = np.inf
    ja[2, rc.L_HIP] = ja[2, rc.R_HIP]                                   # no x axis
    ja[3, rc.NECK] = ja[3, rc.PELVIS] + (ja[3, rc.L_HIP] - ja[3, rc.R_HIP]) * F32(2.0)      # the spine along the hips: no z axis
    jb[4, 9] = ja[4, 9] + F32(4.5)                                      # beyond the cap
    t = rc.shift_terms(ja, jb, F32)
    assert t['good'].tolist() == [False] * 5 + [True]
    table = rc.accumulate(ja, jb, None, 1)
    assert table[rc.COUNT] == 1 and table[rc.BAD] == 5 and not table[-2:].any()
    only = rc.accumulate(ja[5:], jb[5:], None, 1)
    only[rc.BAD] += 5
    assert np.array_equal(table, only)                                  # the five added nothing else
    assert table[rc.HIST:rc.HIST + 17 * 64].sum() == 17


def test_restatement_is_order_free_and_counts_groups_like_the_evaluation_table():
    ja, jb, group = rc.shift_case(67)
    whole = rc.accumulate(ja, jb, group, 3)
    perm = np.random.RandomState(1).permutation(67)
    assert np.array_equal(rc.accumulate(ja[perm], jb[perm], group[perm], 3), whole)
    split = rc.accumulate(ja[1:], jb[1:], group[1:], 3, rc.accumulate(ja[:1], jb[:1], group[:1], 3))
    assert np.array_equal(split, whole)
    rows = whole[:3 * rc.ROW].reshape(3, rc.ROW)
    assert whole[-2] == 2 and whole[-1] == 1 and rows[:, rc.BAD].sum() == 3 and rows[:, rc.COUNT].sum() == 67 - 3 - 3


# ---- 2. derive ----
def _table(poses, n_groups=1):
    """a table from (group, q (17,3) int, length q (17), rel q (17), bins (17)) tuples"""
    t = np.zeros(n_groups * rc.ROW + rc.TRAILER, dtype=np.int64)
    for g, q, ln, rel, bins in poses:
        row = t[g * rc.ROW:(g + 1) * rc.ROW]
        row[rc.COUNT] += 1
        row[rc.SUM:rc.SUM + 51] += q.reshape(-1)
        row[rc.MOM:rc.MOM + 102] += np.stack([(q[:, i] * q[:, k]) >> 16 for i, k in rc.MOM_PAIRS], 1).reshape(-1)
        row[rc.ABS:rc.ABS + 17] += ln
        row[rc.ABS_REL:rc.ABS_REL + 17] += rel
        np.add.at(row, rc.HIST + np.arange(17) * 64 + bins, 1)
    return t


def test_derive_one_pose():
    rr = _mod('regressor_report')
    q = np.zeros((17, 3), dtype=np.int64)
    q[:, 0], q[:, 2] = 1 << 14, -(3 << 14)                               # 2^-10 m = 0.9765625 mm, -3 x that
    ln = np.full(17, 51883, dtype=np.int64)
    res = rr.derive(_table([(0, q, ln, ln // 2, np.full(17, 1))]), ['only'])
    for r in (res['all'], res['groups']['only']):
        assert r['n'] == 1 and r['n_bad'] == 0 and len(r['raw']) == rc.ROW
        assert np.allclose(r['mean_mm'], [[0.9765625, 0, -2.9296875]] * 17, atol=1e-12)
        assert np.array(r['std_mm']).max() == 0                          # one pose: no spread (the dropped fraction only lowers it)
        assert np.allclose(r['mean_abs_mm'], 51883 / 2 ** 24 * 1000, atol=1e-12)
        assert np.allclose(r['mean_abs_pelvis_relative_mm'], (51883 // 2) / 2 ** 24 * 1000, atol=1e-12)
        assert r['median_abs_mm'] == [4.0] * 17 and r['p95_abs_mm'] == [4.0] * 17
    assert res['ignored'] == 0


def test_derive_two_opposite_shifts_mean_zero_std_the_shift():
    rr = _mod('regressor_report')
    q = np.zeros((17, 3), dtype=np.int64)
    q[:, 1] = 5 << 16                                                   # 5 * 2^-8 m = 19.53125 mm; (5 << 16)^2 >> 16 is exact
    poses = [(0, q, q[:, 1], q[:, 1], np.full(17, 9)), (1, -q, q[:, 1], q[:, 1], np.full(17, 9))]
    res = rr.derive(_table(poses, 2), ['a', 'b'])
    assert res['all']['n'] == 2 and res['groups']['a']['n'] == 1
    assert np.abs(np.array(res['all']['mean_mm'])).max() == 0
    std = np.array(res['all']['std_mm'])
    assert np.abs(std[:, 1] - 19.53125).max() <= 1e-12 and std[:, [0, 2]].max() == 0      # (5 << 16)^2 >> 16 drops nothing
    assert np.allclose(res['groups']['b']['mean_mm'], [[0, -19.53125, 0]] * 17, atol=1e-12)
    assert res['all']['median_abs_mm'] == [20.0] * 17


def test_percentiles_of_a_histogram_with_all_mass_in_the_last_bin_and_of_a_spread_one():
    rr = _mod('regressor_report')
    z = np.zeros((17, 3), dtype=np.int64)
    ln = np.full(17, 1 << 22, dtype=np.int64)
    res = rr.derive(_table([(0, z, ln, ln, np.full(17, 63))] * 7), ['g'])['all']
    assert res['median_abs_mm'] == [128.0] * 17 and res['p95_abs_mm'] == [128.0] * 17
    poses = [(0, z, ln, ln, np.full(17, k)) for k in range(20)]         # bins 0 .. 19 once each
    res = rr.derive(_table(poses), ['g'])['all']
    assert res['median_abs_mm'] == [20.0] * 17 and res['p95_abs_mm'] == [38.0] * 17     # the 10th and the 19th of 20 values
    empty = rr.derive(np.zeros(rc.ROW + 2, dtype=np.int64), ['g'])['all']
    assert empty['n'] == 0 and empty['mean_mm'] is None and empty['median_abs_mm'] is None


def test_derive_refuses_a_wrong_table():
    rr = _mod('regressor_report')
    with pytest.raises(ValueError, match='int64 expected for 2 groups'):
        rr.derive(np.zeros(rc.ROW + 2, dtype=np.int64), ['a', 'b'])
    with pytest.raises(ValueError, match='int64 expected'):
        rr.derive(np.zeros(rc.ROW + 2, dtype=np.int32), ['a'])
    with pytest.raises(ValueError, match='int64 expected'):
        rr.derive(np.zeros(338 + 2, dtype=np.int64), ['a'])              # the evaluation report's table
    t = np.zeros(rc.ROW + 2, dtype=np.int64)
    t[-1] = 4
    with pytest.raises(RuntimeError, match='4 poses carried a group id outside'):
        rr.derive(t, ['a'])
    t[-1], t[-2] = 0, 3
    assert rr.derive(t, ['a'])['ignored'] == 3


def test_shift_report_on_cpu_tensors_refuses_what_the_device_kernel_cannot_take():
    rr = _mod('regressor_report')
    rep = rr.ShiftReport(['a', 'b'], 'cpu')
    assert rep.acc.shape == (2 * rc.ROW + 2,) and rep.acc.dtype == torch.int64
    assert rep.finish(reduce=False)['all']['n'] == 0
    with pytest.raises(ValueError, match='groups'):
        rr.ShiftReport([], 'cpu')
    with pytest.raises(ValueError, match='int32 tensor on'):
        rep.add(torch.zeros(2, 17, 3), torch.zeros(2, 17, 3), torch.zeros(2, dtype=torch.int64))


# ---- 3. the flags ----
def test_flags_default_to_off_and_are_checked(tmp_path):
    a, rr = _mod('args'), _mod('regressor_report')
    ns = a.get_args([])
    assert ns.regressor_report is None and ns.regressor_report_images == 8 and ns.regressor_report_size == 256
    rr.check_flags(ns)
    rr.check_flags(a.get_args(['--regressor_report_size', '100']))      # without the report nothing is checked
    ns = a.get_args(['--regressor_report', 'out', '--regressor_report_images', '3', '--regressor_report_size', '224'])
    assert (ns.regressor_report, ns.regressor_report_images, ns.regressor_report_size) == ('out', 3, 224)
    rr.check_flags(ns)
    for bad in ('100', '0', '288'):
        with pytest.raises(ValueError, match='a size the rasteriser takes'):
            rr.check_flags(a.get_args(['--regressor_report', 'out', '--regressor_report_size', bad]))
    with pytest.raises(ValueError, match='--regressor_report_images'):
        rr.check_flags(a.get_args(['--regressor_report', 'out', '--regressor_report_images', '-1']))


def _vertices_dir(tmp_path):
    d = tmp_path / 'in'
    d.mkdir()
    np.save(d / 'vertices.npy', np.zeros((2, 6890, 3), dtype=F32))
    np.save(d / 'gt_j3d.npy', np.zeros((2, 17, 3), dtype=F32))
    return str(d)


def test_eval_vertices_needs_one_of_the_two_reports(tmp_path):
    er = _mod('eval_report')
    good = _vertices_dir(tmp_path)
    with pytest.raises(ValueError, match='--eval_vertices needs --eval_report or --regressor_report'):
        _with_args(['--eval_vertices', good, '--synthetic'], er.evaluate_vertices)
    # with the regressor report alone the flags pass: the next refusal is the report's own size check, before any launch
    with pytest.raises(ValueError, match='a size the rasteriser takes'):
        _with_args(['--eval_vertices', good, '--synthetic', '--regressor_report', str(tmp_path / 'out'), '--regressor_report_size', '100'],
                   er.evaluate_vertices)


def test_body_model_for_the_pictures_only_when_one_is_available(tmp_path):
    rr = _mod('regressor_report')
    assert rr.resolve_body_model(str(tmp_path), False) is None and rr.resolve_body_model(None, False) is None
    m = rr.resolve_body_model(str(tmp_path), True)
    assert m['faces'].shape[1] == 3 and m['v_template'].shape == (6890, 3) and m['provenance'].startswith('synthetic')


# ---- 4. frame_camera ----
def _project(verts, cam, S):
    """the rasteriser's projection (include/jrr.h, jrr_mesh_shade step 1) in float64: NDC u, v"""
    v, c = verts.double(), cam.double()
    F = 5000.0 / S
    Z = 2 * v[..., 2] + c[:, None, 2]
    return F * (-2 * v[..., 0] + c[:, None, 0]) / Z, F * (-2 * v[..., 1] + c[:, None, 1]) / Z, Z


@pytest.mark.parametrize('S', [32, 256])
def test_frame_camera_keeps_every_vertex_inside_and_fills_half_the_picture(S, smpl_model_np):
    report, rr = _mod('report'), _mod('regressor_report')
    g = torch.Generator().manual_seed(S)
    random = torch.randn(5, 300, 3, generator=g) * torch.tensor([0.3, 0.6, 0.15]) + torch.randn(5, 1, 3, generator=g) * 2.0
    random[3] = random[3, :, [1, 0, 2]]                                  # a body wider than tall
    body = torch.from_numpy(smpl_model_np['v_template'].astype(F32))[None]
    for verts in (random, body, report.side_view(body, torch.zeros(1, 3))):
        cam = report.frame_camera(verts, S)
        assert cam.shape == (verts.shape[0], 3) and cam.dtype == verts.dtype
        u, v, Z = _project(verts, cam, S)
        assert (Z > 0).all() and u.abs().max() <= 0.9 + 1e-5 and v.abs().max() <= 0.9 + 1e-5
        xy = rr.project_points(verts, cam, S).double()                   # as pixels: inside [-0.5, S - 0.5]
        assert xy.min() >= -0.5 and xy.max() <= S - 0.5
        extent = torch.maximum(u.max(1).values - u.min(1).values, v.max(1).values - v.min(1).values) / 2.0
        assert (extent >= 0.5).all() and (extent <= 0.9 + 1e-5).all(), extent
    # the pixel map is the rasteriser's: NDC +1 is the left / upper edge of pixel 0, NDC 0 the middle of the picture
    cam = torch.tensor([[0.0, 0.0, 50.0]])
    assert torch.allclose(rr.project_points(torch.zeros(1, 1, 3), cam, S), torch.full((1, 1, 2), (S - 1) / 2.0))
    with pytest.raises(ValueError):
        report.frame_camera(body[0], S)
    with pytest.raises(ValueError):
        report.frame_camera(body, S, margin=1.0)
    one = report.frame_camera(torch.zeros(1, 4, 3), S)                   # a pose of zero extent still gets a finite camera
    assert torch.isfinite(one).all() and one[0, 2] > 0


def test_side_view_turns_other_points_with_the_vertices():
    report = _mod('report')
    g = torch.Generator().manual_seed(4)
    verts, cam = torch.randn(2, 40, 3, generator=g), torch.zeros(2, 3)
    turned = report.side_view(verts, cam)
    part = report.side_view(verts[:, :7], cam, centre=verts.mean(dim=1, keepdim=True))
    assert torch.equal(part, turned[:, :7])
    with pytest.raises(ValueError):
        report.side_view(verts, cam, centre=verts.mean(dim=1))


# ---- 5. the two regressors without data ----
def test_compare_regressors_counts_and_template_shift(smpl_model_np):
    rr, sm = _mod('regressor_report'), _mod('smpl_model')
    J = sm.default_h36m_regressor()
    J2 = (J * (1 + 0.5 * np.random.RandomState(5).rand(*J.shape))).astype(F32)
    J2[3, np.flatnonzero(J[3] > 0)[0]] = -1.0                            # one vertex leaves the support of joint 3
    J2[3, 17] = 0.25                                                     # and one joins it
    mask = np.ones_like(J)
    vt = smpl_model_np['v_template']
    rows = rr.compare_regressors(J, J2, mask, vt)
    A, B = rr.normalised(J, mask), rr.normalised(J2, mask)
    assert np.allclose(A.sum(1), 1) and np.allclose(B.sum(1), 1) and (A >= 0).all()
    for j, r in enumerate(rows):
        assert r['joint'] == _mod('eval_report').JOINT_NAMES[j]
        assert r['support_a'] == int((J[j] > 0).sum()) and r['support_b'] == int((J2[j] > 0).sum())
        assert r['shared'] == int(((J[j] > 0) & (J2[j] > 0)).sum())
        assert abs(r['l1'] - np.abs(A[j] - B[j]).sum()) <= 1e-15
        want = (B[j] - A[j]) @ vt.astype(F64)
        assert np.abs(np.array(r['template_shift_mm']) / 1000 - want).max() <= 1e-9
        assert [t['vertex'] for t in r['top_a']] == np.lexsort((np.arange(6890), -A[j]))[:min(5, r['support_a'])].tolist()
        assert all(t['weight'] > 0 for t in r['top_b']) and len(r['top_b']) == min(5, r['support_b'])
    assert rows[3]['shared'] == rows[3]['support_a'] - 1 and rows[3]['support_b'] == rows[3]['support_a']
    same = rr.compare_regressors(J, J, mask)
    assert all(r['l1'] == 0 and r['template_shift_mm'] is None for r in same)


def test_files_are_written_by_rank_zero_and_read_back(tmp_path):
    rr = _mod('regressor_report')
    ja, jb, group = rc.shift_case(67)
    group[group == 3] = 0
    data = rr.derive(rc.accumulate(ja, jb, group, 3), ['Walking', 'Sitting', 'Eating'])
    J = _mod('smpl_model').default_h36m_regressor()
    joints = rr.compare_regressors(J, J * F32(2.0))
    doc = rr.write(str(tmp_path), data, joints, ['Walking', 'Sitting', 'Eating'], 'vertices', {'batch_size': 8}, ('a.npy', '0' * 16),
                   ('b.pt', '1' * 16), 'skipped: no body model')
    assert sorted(os.listdir(tmp_path)) == ['regressor.json', 'regressor.md']
    back = rr.load(str(tmp_path))
    assert back['pictures'] == 'skipped: no body model' and back['source'] == 'vertices' and back['layout_version'] == 1
    assert back['data'] == doc['data'] and back['data']['all']['n'] == 62 and back['data']['ignored'] == 2
    assert back['j_regressor_retrained'] == {'path': 'b.pt', 'sha256_16': '1' * 16} and len(back['joints']) == 17
    md = open(tmp_path / 'regressor.md', encoding='utf-8').read()
    assert '| L_Wrist |' in md and '| Sitting |' in md and 'green' in md and 'blue' in md and 'red' in md


# ---- 6. the evaluation driver's engine calls, with and without the flag ----
class _FakeEngine:
    log = []

    def __init__(self, model, batch, *args, **kwargs):
        self.batch = batch
        _FakeEngine.log.append(('RefineEngine', model, batch, args, tuple(sorted(kwargs.items()))))

    def set_j_regressor(self, J, mask=None):
        _FakeEngine.log.append(('set_j_regressor', tuple(J.shape), None if mask is None else tuple(mask.shape)))

    def find_joints_forward(self, betas, *args, **kwargs):
        _FakeEngine.log.append(('find_joints_forward', args, tuple(sorted(k for k, v in kwargs.items() if v is not None and v is not False))))
        joints = torch.zeros(self.batch, 17, 3)
        return (joints, torch.zeros(self.batch, 6890, 3)) if kwargs.get('return_verts') else joints


class _FakeSMPL:
    def __init__(self, *a, **k):
        self.model_np = {'v_template': np.zeros((6890, 3), dtype=F32), 'faces': None}
        self.device_model, self.provenance = 'device-model', 'fake'

    def to(self, device):
        return self


class _FakeRun:
    log = []

    def __init__(self, ns, names, device, J_a, J_b, mask, source):
        _FakeRun.log.append(('Run', list(names), source, J_a.shape, J_b.shape))

    def add(self, verts, ja, jb, gt, gid, scored=None):
        _FakeRun.log.append(('add', tuple(verts.shape), tuple(ja.shape), tuple(jb.shape), gid.dtype))

    def finish(self, initial, retrained, model_np=None, device_model=None, reduce=True, log=print):
        _FakeRun.log.append(('finish', device_model, reduce))
        return {'fake': True}


def _driver_calls(monkeypatch, tmp_path, extra):
    ev = _mod('test')
    J = _mod('smpl_model').default_h36m_regressor()
    ck = str(tmp_path / 'retrained.pt')
    _mod('checkpoint').save_j_regressor(torch.from_numpy(J * F32(1.5)), ck)
    _FakeEngine.log, _FakeRun.log = [], []
    monkeypatch.setattr(ev, 'SMPL', _FakeSMPL)
    monkeypatch.setattr(ev._engine, 'RefineEngine', _FakeEngine)
    monkeypatch.setattr(ev.utils, 'evaluate', lambda joints, gt: (1.0, 2.0))
    monkeypatch.setattr(ev.regressor_report, 'Run', _FakeRun)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    batch = {'pose6d': torch.zeros(4, 24, 6), 'betas': torch.zeros(4, 10), 'gt_j3d': torch.zeros(4, 17, 3)}
    monkeypatch.setattr(ev, 'validation_batches', lambda model_np, J_np, device, with_index=False: iter([dict(batch), dict(batch)]))
    lines = []
    rep = _with_args(['--device', 'cpu', '--synthetic', '--eval_j_regressor', ck, '--batch_size', '4'] + extra,
                     lambda: ev.test_pose_refiner_model(log=lines.append))
    return rep, lines, list(_FakeEngine.log), list(_FakeRun.log)


TODAY = [('RefineEngine', 'device-model', 4, (), ())] + [
    ('set_j_regressor', (17, 6890), (17, 6890)), ('find_joints_forward', (), ('x6d',)),
    ('set_j_regressor', (17, 6890), (17, 6890)), ('find_joints_forward', (), ('x6d',))] * 2


def test_without_the_flag_the_driver_issues_exactly_todays_calls(monkeypatch, tmp_path):
    rep, lines, calls, run = _driver_calls(monkeypatch, tmp_path, [])
    assert calls == TODAY and run == [] and 'regressor_report' not in rep and len(lines) == 10
    assert os.listdir(tmp_path) == ['retrained.pt']                      # and writes no file


def test_with_the_flag_the_driver_keeps_the_vertices_of_its_first_forward(monkeypatch, tmp_path):
    eng = _mod('engine')
    plain = _driver_calls(monkeypatch, tmp_path, [])[1]
    rep, lines, calls, run = _driver_calls(monkeypatch, tmp_path, ['--regressor_report', str(tmp_path / 'out')])
    assert lines == plain and rep['regressor_report'] == {'fake': True}
    want = [('RefineEngine', 'device-model', 4, (), (('flags', eng.FLAG_KEEP_VERTS),))] + [
        ('set_j_regressor', (17, 6890), (17, 6890)), ('find_joints_forward', (), ('return_verts', 'x6d')),
        ('set_j_regressor', (17, 6890), (17, 6890)), ('find_joints_forward', (), ('x6d',))] * 2
    assert calls == want                                                 # no third forward: the vertices do not depend on the regressor
    assert run == [('Run', ['all'], 'parameters', (17, 6890), (17, 6890))] + [('add', (4, 6890, 3), (4, 17, 3), (4, 17, 3), torch.int32)] * 2 + [
        ('finish', 'device-model', False)]
