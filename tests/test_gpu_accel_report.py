"""The acceleration error along each video sequence on the GPU (pytest -m gpu): jrr_accel_error against the float64 evaluation of the
host restatement (tests/accel_cases.py), the properties the header promises, and the three places `--eval_accel` takes effect.

Bounds: there is no reference implementation, so the per-position outputs are held to `3 x (distance of the restatement's float32
evaluation from its float64 evaluation on THIS test's inputs) + 1e-7` (accel_cases.bound), the maximum over all entries.  The int64
table is held EXACTLY to the host-side integer accumulation of the float32 rows the same call wrote.

Shapes: a 96-row table, 70 listed rows in a non-monotone order, runs of 3, 33, 1, 9, 2, 4 and 18 positions (three workgroups of 32
positions, the last with 6; the run of 33 straddles the border of the first two), three groups with more than one in the first tile
and a single one in the last, one position with group -1 and one with group 3.
"""
import importlib
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import accel_cases as ac
from conftest import PKG_NAME, ROOT

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
F, F64 = np.float32, np.float64
WORDS = ac.N_GROUPS * ac.ROW + ac.TRAILER


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Case:
    """accel_cases.motion_case on the device, with what the restatement says about it (computed once, never changed)"""

    def __init__(self):
        self.pred_np, self.gt_np, self.order_np, self.run_np, self.group_np = ac.motion_case()
        self.pred, self.gt = T(self.pred_np).to(DEV), T(self.gt_np).to(DEV)
        self.order, self.run, self.group = T(self.order_np).to(DEV), T(self.run_np).to(DEV), T(self.group_np).to(DEV)
        self.has, _ = ac.triples(self.order_np, self.run_np, ac.N_ROWS)
        self.r64 = ac.accel(self.pred_np, self.gt_np, self.order_np, self.run_np, F64)
        self.r32 = ac.accel(self.pred_np, self.gt_np, self.order_np, self.run_np, F)
        self.bounds = [ac.bound(a, b) for a, b in zip(self.r32, self.r64)]

    def call(self, pred=None, gt=None, order=None, run=None, group='case', n_groups=ac.N_GROUPS, acc='new', **kw):
        """(rows as numpy or None, table as numpy or None, status)"""
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        group = self.group if isinstance(group, str) else group
        if isinstance(acc, str):
            acc = torch.zeros(n_groups * ac.ROW + ac.TRAILER, dtype=torch.int64, device=DEV)
        out = _mod('engine').accel_error(self.pred if pred is None else pred, self.gt if gt is None else gt,
                                         self.order if order is None else order, self.run if run is None else run, status, group=group,
                                         n_groups=n_groups, acc=acc, **kw)
        return (None if out is None else [t.cpu().numpy() for t in out], None if acc is None else acc.cpu().numpy(), int(status.item()))


@pytest.fixture(scope='module')
def case():
    return Case()


@pytest.fixture(scope='module')
def whole(case):
    """one call over [0, M): what every other call is compared with"""
    return case.call()


# ---- 1. the kernel against float64, and its table against its own rows ----
def test_rows_against_float64_and_nan_exactly_without_a_triple(case, whole):
    before = (case.pred.clone(), case.gt.clone())
    rows, table, status = case.call()
    assert status == 0
    for name, got, want, b in zip(('e', 's', 'g'), rows, case.r64, case.bounds):
        d = ac.dist(got, want)
        print(f'{name}: {d:.3e} (bound {b:.3e}); bits equal to the float32 restatement: {np.array_equal(_bits(got), _bits(case.r32["esg".index(name)]))}')
        assert got.dtype == F and got.shape == (ac.M, 17)
        assert np.array_equal(np.isnan(got), np.broadcast_to(~case.has[:, None], (ac.M, 17)))
        assert d <= b
    assert not rows[0][case.has, 0].any() and rows[0][case.has, 1:].min() > 0          # the pelvis: 0 by definition; the others moved
    assert torch.equal(case.pred.view(torch.int32), before[0].view(torch.int32)) and torch.equal(case.gt.view(torch.int32), before[1].view(torch.int32))
    for a, b in zip(rows, whole[0]):
        assert np.array_equal(_bits(a), _bits(b))                                   # a second call: the same bits


def test_table_is_exactly_the_integer_accumulation_of_the_rows_it_wrote(case, whole):
    rows, table, status = whole
    want = ac.accumulate(rows[0], rows[1], rows[2], case.has, case.group_np, ac.N_GROUPS)
    assert table.dtype == np.int64 and table.shape == (WORDS,) and np.array_equal(table, want)
    t = table[:-2].reshape(ac.N_GROUPS, ac.ROW)
    assert table[-2:].tolist() == [1, 1]                                             # one ignored, one with a group outside
    assert int(t[:, ac.COUNT].sum()) == int(case.has.sum()) - 2 and int(t[:, ac.NO_TRIPLE].sum()) == ac.M - int(case.has.sum())
    assert not t[:, ac.BAD].any() and (t[:, ac.COUNT] > 0).all()
    assert int(t[:, ac.HIST:ac.HIST + ac.BINS].sum()) == 17 * int(t[:, ac.COUNT].sum())
    # no groups given: everything in group 0, the trailer empty; no table asked for: the same rows; no rows asked for: the same table
    rows0, table0, _ = case.call(group=None, n_groups=1)
    assert np.array_equal(table0, ac.accumulate(rows0[0], rows0[1], rows0[2], case.has, None, 1)) and table0[-2:].tolist() == [0, 0]
    assert int(table0[ac.COUNT]) == int(case.has.sum())
    rows1, none, _ = case.call(acc=None)
    assert none is None and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(rows1, rows)) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(rows0, rows))
    none, table2, _ = case.call(rows=False)
    assert none is None and np.array_equal(table2, table)
    # the derived numbers are the float64 restatement's means, to the bound
    with pytest.raises(RuntimeError, match='1 positions carried a group id outside'):
        _mod('accel_report').derive(table, ['a', 'b', 'c'])                          # the caller's error is reported, not averaged away
    clean = table.copy()
    clean[-1] = 0
    doc = _mod('accel_report').derive(clean, ['a', 'b', 'c'])
    counted = case.has & (case.group_np >= 0) & (case.group_np < ac.N_GROUPS)
    assert abs(doc['all']['accel_err_mm'] - case.r64[0][counted].mean() * 1000) <= 1000 * (case.bounds[0] + 2.0 ** -25)
    assert doc['ignored'] == 1


# ---- 2. what the header promises ----
def test_range_and_tiling_leave_every_bit_alone(case, whole):
    rows, table, _ = whole
    engine = _mod('engine')
    # two halves, split inside the run of 33 (positions 3 .. 35) and away from a multiple of the tile
    cut = 20
    assert case.run_np[cut - 1] == case.run_np[cut] == 1
    out = tuple(torch.full((ac.M, 17), float('nan'), device=DEV) for _ in range(3))
    halves = []
    for b, c in ((0, cut), (cut, ac.M - cut)):
        _, t, st = case.call(begin=b, count=c, out=out)
        assert st == 0
        halves.append(t)
    assert all(np.array_equal(_bits(a.cpu().numpy()), _bits(b)) for a, b in zip(out, rows))
    assert np.array_equal(halves[0] + halves[1], table) and halves[0].any() and halves[1].any()
    # single positions, all into one table: rows outside a call's range are not touched (they keep the marker)
    out = tuple(torch.full((ac.M, 17), -7.0, device=DEV) for _ in range(3))
    acc = torch.zeros(WORDS, dtype=torch.int64, device=DEV)
    _, _, st = case.call(begin=40, count=1, out=out, acc=acc)
    first = [t.cpu().numpy() for t in out]
    assert all((a[:40] == -7).all() and (a[41:] == -7).all() and np.array_equal(_bits(a[40]), _bits(b[40])) for a, b in zip(first, rows))
    for p in list(range(40)) + list(range(41, ac.M)):
        case_status = torch.zeros(1, dtype=torch.int32, device=DEV)
        engine.accel_error(case.pred, case.gt, case.order, case.run, case_status, group=case.group, n_groups=ac.N_GROUPS, acc=acc, begin=p, count=1,
                           out=out)
    assert all(np.array_equal(_bits(a.cpu().numpy()), _bits(b)) for a, b in zip(out, rows))
    assert np.array_equal(acc.cpu().numpy(), table)
    # an empty range launches nothing
    _, t, _ = case.call(begin=ac.M, count=0)
    assert not t.any()


def test_a_permuted_run_order_gives_the_same_table(case, whole):
    rows, table, _ = whole
    starts = np.concatenate([[0], np.cumsum(ac.RUN_LENGTHS)])
    blocks = [np.arange(starts[r], starts[r + 1]) for r in (4, 1, 6, 0, 3, 5, 2)]       # the runs in another order, each in its own
    perm = np.concatenate(blocks)
    assert perm[:2].tolist() == [46, 47] and sorted(perm.tolist()) == list(range(ac.M))
    got, t, st = case.call(order=T(case.order_np[perm]).to(DEV), run=T(case.run_np[perm]).to(DEV), group=T(case.group_np[perm]).to(DEV))
    assert st == 0 and np.array_equal(t, table)
    for a, b in zip(got, rows):
        assert np.array_equal(_bits(a), _bits(b[perm]))                              # every position keeps its bits, wherever its tile


def test_status_bit_0_for_an_order_entry_outside_the_table(case, whole):
    rows, table, _ = whole
    order = case.order_np.copy()
    order[20], order[60] = ac.N_ROWS, -1
    got, t, st = case.call(order=T(order).to(DEV))
    assert st == 1
    hit = np.zeros(ac.M, bool)
    hit[[19, 20, 21, 59, 60, 61]] = True                                            # absent: no triple of its own, nobody's neighbour
    has, absent = ac.triples(order, case.run_np, ac.N_ROWS)
    assert np.array_equal(has, case.has & ~hit) and absent.sum() == 2
    for a, b in zip(got, rows):
        assert np.isnan(a[hit]).all() and np.array_equal(_bits(a[~hit]), _bits(b[~hit]))
    assert np.array_equal(t, ac.accumulate(got[0], got[1], got[2], has, case.group_np, ac.N_GROUPS))
    assert int(t[:-2].reshape(3, ac.ROW)[:, ac.NO_TRIPLE].sum()) == ac.M - int(case.has.sum()) + 6


def test_a_nan_row_makes_exactly_the_triples_that_hold_it_bad(case, whole):
    rows, table, _ = whole
    pred, gt = case.pred.clone(), case.gt.clone()
    pred[int(case.order_np[20]), 3, 1] = float('nan')                               # one component of one joint of position 20
    gt[int(case.order_np[60]), 0, 2] = float('inf')                                 # the pelvis of position 60: every joint of its frame
    got, t, st = case.call(pred=pred, gt=gt)
    assert st == 0
    hit = np.zeros(ac.M, bool)
    hit[[19, 20, 21, 59, 60, 61]] = True
    assert case.has[hit].all() and (case.group_np[hit] >= 0).all() and (case.group_np[hit] < ac.N_GROUPS).all()
    for a, b in zip(got, rows):
        assert np.array_equal(_bits(a[~hit]), _bits(b[~hit]))
    assert np.isnan(got[0][[19, 20, 21], 3]).all() and np.isnan(got[1][[19, 20, 21], 3]).all() and np.isfinite(got[0][[19, 20, 21], 4]).all()
    assert np.array_equal(_bits(got[2][19:22]), _bits(rows[2][19:22]))              # the ground truth's own acceleration there is untouched
    assert not np.isfinite(got[0][59:62]).any() and not np.isfinite(got[2][59:62]).any() and np.array_equal(_bits(got[1][59:62]), _bits(rows[1][59:62]))
    tt, t0 = t[:-2].reshape(3, ac.ROW), table[:-2].reshape(3, ac.ROW)
    assert int(tt[:, ac.BAD].sum()) == 6 and int(tt[:, ac.COUNT].sum()) == int(t0[:, ac.COUNT].sum()) - 6
    assert np.array_equal(tt[:, ac.NO_TRIPLE], t0[:, ac.NO_TRIPLE]) and np.array_equal(t[-2:], table[-2:])
    assert np.array_equal(t, ac.accumulate(got[0], got[1], got[2], case.has, case.group_np, ac.N_GROUPS))


# ---- 3. the three places of --eval_accel ----
def _with_args(flags, fn):
    argsmod = _mod('args')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(flags + ['--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent', '--synthetic', '--device', DEV])
    try:
        torch.manual_seed(0)
        return fn()
    finally:
        argsmod._LazyArgs._ns = saved


def _rig_paths(n=40):
    """two cameras interleaved in file order, camera 1 skips one frame; the last sample is a stray without imageSequence"""
    cam_of = np.arange(n) % 2
    frame = 5 * (np.arange(n) // 2 + 1)
    frame[cam_of == 0] += np.where(np.arange(n // 2) >= 12, 5, 0)                   # camera 1 skips frame 65
    paths = [f'/data/h36m/S9/Walking 1/imageSequence/{c + 1}/img_{f:06d}.jpg' for c, f in zip(cam_of, frame)]
    paths[n - 1] = '/data/elsewhere/000001.jpg'
    return paths, cam_of


def _write_dataset(root, tensors, paths):
    d = os.path.join(root, 'precomputed_val')
    os.makedirs(d)
    for k, v in tensors.items():
        torch.save(v, os.path.join(d, f'{k}.pt'))
    with open(os.path.join(d, 'images.pkl'), 'wb') as f:
        pickle.dump(paths, f)


def _checkpoint(tmp):
    J = _mod('smpl_model').default_h36m_regressor()
    J2 = (J * (1 + 0.5 * np.random.RandomState(5).rand(*J.shape))).astype(F)               # a regressor that differs from the initial one
    ck = os.path.join(tmp, 'retrained_J_Regressor.pt')
    _mod('checkpoint').save_j_regressor(T(J2), ck)
    return ck, J, J2


def test_eval_accel_through_test_pose_refiner_model(tmp_path, smpl_model_np, j_h36m_np):
    """a 40-sample dataset directory with a camera rig, batches of 20: accel.json beside an eval.json that keeps its bytes"""
    n = 40
    root = str(tmp_path / 'data')
    os.makedirs(root)
    paths, cam_of = _rig_paths(n)
    rng = np.random.RandomState(3)
    full = _mod('smpl_model').synthetic_batch(smpl_model_np, j_h36m_np, n, seed=0)
    aa = (rng.normal(0, 0.3, size=(2, 24, 3))[cam_of] + 0.02 * (np.arange(n) // 2)[:, None, None] + rng.normal(0, 0.03, size=(n, 24, 3))).astype(F)
    _write_dataset(root, {'bboxes': torch.tensor([[100., 200., 700., 800.]]).repeat(n, 1), 'betas': T(full['betas']),
                          'estimated_translation': T(full['cam']), 'gt_j2d': torch.rand(n, 17, 2) * 1000, 'gt_j3d': T(full['gt_j3d']),
                          'intrinsics': torch.eye(3).repeat(n, 1, 1), 'orient': T(aa[:, 0]), 'pose': T(aa[:, 1:].reshape(n, 69))}, paths)
    ck, _, _ = _checkpoint(str(tmp_path))
    evaluation, ar = _mod('test'), _mod('accel_report')
    flags = ['--batch_size', '20', '--data_root', root, '--eval_j_regressor', ck]
    runs = {}
    for key, extra in (('plain', []), ('accel', ['--eval_accel'])):
        lines = []
        out = str(tmp_path / key)
        rep = _with_args(flags + ['--eval_report', out] + extra, lambda: evaluation.test_pose_refiner_model(log=lines.append))
        runs[key] = (out, lines, rep)
    (out0, lines0, rep0), (out1, lines1, rep1) = runs['plain'], runs['accel']
    assert sorted(os.listdir(out0)) == ['eval.json', 'eval.md'] and sorted(os.listdir(out1)) == ['accel.json', 'accel.md', 'eval.json', 'eval.md']
    for name in ('eval.md',):
        assert open(os.path.join(out0, name), 'rb').read() == open(os.path.join(out1, name), 'rb').read()
    e0, e1 = (json.load(open(os.path.join(o, 'eval.json'))) for o in (out0, out1))
    assert e0['flags'].pop('eval_report') == out0 and e1['flags'].pop('eval_report') == out1 and e0 == e1 and 'eval_accel' not in e0['flags']
    assert lines1[:-1] == lines0 and lines1[-1].startswith('acceleration error, mm per sampled frame^2: before ') and 'accel_report' not in rep0
    doc = ar.load(out1)
    order, run, frame = _mod('refined').sequence_runs(paths, np.ones(n, bool))
    assert np.bincount(run).tolist() == [12, 8, 19, 1]
    assert doc['source'] == 'parameters' and doc['groups'] == ['Walking', 'all'] and doc['rows'] == n and doc['present'] == n
    assert doc['split'] == {'positions': 40, 'runs': 4, 'run_length_histogram': {'1': 1, '8': 1, '12': 1, '19': 1}, 'stride_histogram': {'5': 3}}
    for which in ('before', 'after'):
        r = doc['sets'][which]
        assert r['all']['n'] == 10 + 6 + 17 and r['all']['n_no_triple'] == 7 and r['all']['n_bad'] == 0 and r['ignored'] == 0
        assert r['groups']['Walking']['n'] == 33 and r['groups']['all']['n_no_triple'] == 1 and r['all']['accel_err_mm'] > 0
        print(f"{which}: accel error {r['all']['accel_err_mm']:.4f} mm/frame^2, |a_pred| {r['all']['accel_pred_mm']:.4f}, |a_gt| {r['all']['accel_gt_mm']:.4f}")
    assert doc['sets']['before']['all']['raw'] != doc['sets']['after']['all']['raw']
    assert doc['sets']['before']['all']['accel_gt_mm'] == doc['sets']['after']['all']['accel_gt_mm']        # one ground truth


def test_eval_accel_through_eval_vertices_two_gloo_ranks_equal_one(tmp_path, smpl_model_np):
    """40 meshes of two cameras: main.py --eval_vertices under torchrun, two ranks over gloo sharing cuda:0, writes the accel.json bytes
    of one rank"""
    n = 40
    tmp = str(tmp_path)
    ck, J, _ = _checkpoint(tmp)
    paths, cam_of = _rig_paths(n)
    rng = np.random.RandomState(11)
    t = (np.arange(n) // 2)[:, None, None]
    verts = (smpl_model_np['v_template'][None] + 0.01 * t * rng.normal(0, 1, size=(1, 1, 3)) + 0.02 * np.sin(0.4 * t + rng.uniform(0, 6, size=(1, 6890, 3)))
             + rng.normal(0, 0.002, size=(n, 6890, 3))).astype(F)
    vdir = os.path.join(tmp, 'meshes')
    os.makedirs(vdir)
    np.save(os.path.join(vdir, 'vertices.npy'), verts)
    np.save(os.path.join(vdir, 'gt_j3d.npy'), (np.einsum('jv,nvc->njc', J.astype(F64), verts.astype(F64)) * 1000 + rng.normal(0, 3, size=(n, 17, 3))).astype(F))
    with open(os.path.join(vdir, 'paths.txt'), 'w') as f:
        f.write('\n'.join(paths) + '\n')
    flags = ['--batch_size', '16', '--eval_j_regressor', ck, '--eval_vertices', vdir, '--eval_accel']
    one = os.path.join(tmp, 'one')
    lines = []
    _with_args(flags + ['--eval_report', one], lambda: _mod('eval_report').evaluate_vertices(log=lines.append))
    assert sorted(os.listdir(one)) == ['accel.json', 'accel.md', 'eval.json', 'eval.md'] and len(lines) == 4 and lines[2].startswith('acceleration error')
    doc = _mod('accel_report').load(one)
    assert doc['source'] == 'vertices' and doc['sets']['before']['all']['n'] == 33 and doc['sets']['after']['all']['n_no_triple'] == 7
    assert doc['sets']['before']['all']['accel_err_mm'] > 0 and doc['sets']['before']['all']['raw'] != doc['sets']['after']['all']['raw']
    with pytest.raises(ValueError, match=r'paths\.txt is missing'):
        os.rename(os.path.join(vdir, 'paths.txt'), os.path.join(vdir, 'paths.off'))
        try:
            _with_args(flags + ['--eval_report', os.path.join(tmp, 'never')], lambda: _mod('eval_report').evaluate_vertices(log=lines.append))
        finally:
            os.rename(os.path.join(vdir, 'paths.off'), os.path.join(vdir, 'paths.txt'))
    assert not os.path.exists(os.path.join(tmp, 'never'))
    two = os.path.join(tmp, 'two')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1', '--master-port', '29589',
           os.path.join(ROOT, 'main.py')] + flags + ['--eval_report', two, '--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent', '--synthetic',
                                                     '--device', DEV, '--single_device', '--dist_backend', 'gloo']
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert sorted(os.listdir(two)) == ['accel.json', 'accel.md', 'eval.json', 'eval.md']
    for name in ('accel.json', 'accel.md'):
        assert open(os.path.join(two, name), 'rb').read() == open(os.path.join(one, name), 'rb').read(), name


def test_eval_accel_through_smooth_command_smoothing_lowers_the_error(tmp_path):
    """40 frames of one camera: noisy poses planted around a smooth ground-truth motion; the ground-truth joints are the true poses'
    joints through the same body and regressor"""
    n = 40
    refined, eng, sm = _mod('refined'), _mod('engine'), _mod('smpl_model')
    SMPL = _mod('smpl').SMPL
    root, out_dir = str(tmp_path / 'data'), str(tmp_path / 'refined')
    os.makedirs(root)
    rng = np.random.RandomState(8)
    t = np.arange(n, dtype=F64)[:, None, None]
    aa_true = rng.normal(0, 0.3, size=(1, 24, 3)) + 0.15 * np.sin(0.12 * t + rng.uniform(0, 6, size=(1, 24, 3)))
    aa_noisy = aa_true + rng.normal(0, 0.03, size=(n, 24, 3))
    to6d = lambda aa: eng.rodrigues_forward(T(aa.astype(F)).to(DEV).reshape(-1, 3)).reshape(n, 24, 3, 3)[..., :2].reshape(n, 24, 6).contiguous()
    betas = T(np.tile(rng.normal(0, 0.5, size=(1, 10)).astype(F), (n, 1))).to(DEV)
    smpl = SMPL('/nonexistent', batch_size=1, allow_synthetic=True).to(DEV)
    J = T(sm.default_h36m_regressor('/nonexistent', allow_default=True)).float().to(DEV)
    engine = eng.RefineEngine(smpl.device_model, n)
    engine.set_j_regressor(J, _mod('utils').find_j_reg_mask(J))
    gt_mm = (engine.find_joints_forward(betas, x6d=to6d(aa_true)).float() * 1000).cpu()
    paths = [f'/data/h36m/S9/Walking/imageSequence/1/img_{f:06d}.jpg' for f in range(1, n + 1)]
    _write_dataset(root, {'bboxes': torch.tensor([[100., 200., 700., 800.]]).repeat(n, 1), 'betas': betas.cpu(), 'estimated_translation': torch.zeros(n, 3),
                          'gt_j2d': torch.rand(n, 17, 2) * 1000, 'gt_j3d': gt_mm, 'intrinsics': torch.eye(3).repeat(n, 1, 1),
                          'orient': T(aa_noisy[:, 0].astype(F)), 'pose': T(aa_noisy[:, 1:].reshape(n, 69).astype(F))}, paths)
    table = refined.RefinedTable(n, DEV)
    table.add(torch.arange(n, dtype=torch.int64, device=DEV), to6d(aa_noisy), betas, torch.zeros(n, 3, device=DEV))
    table.finish(out_dir, {'inner_iters': 0, 'data': 'dataset'})
    lines = []
    flags = ['--smooth_refined', out_dir, '--data_root', root, '--batch_size', '24']
    plain = _with_args(flags, lambda: refined.smooth_command(log=lines.append))
    assert not [k for k in plain if k.startswith('accel')] and 'accel error' not in lines[0]
    out = _with_args(flags + ['--eval_accel'], lambda: refined.smooth_command(log=lines.append))
    back = refined.load(out_dir, n=n, name='refined_smooth.npz')
    s = back['meta']['smooth']
    for name in ('accel_err_mm_raw', 'accel_err_mm_smooth'):
        a = back[name]
        assert a.shape == (n,) and a.dtype == F and np.isnan(a[[0, n - 1]]).all() and np.isfinite(a[1:n - 1]).all() and np.array_equal(a, out[name], equal_nan=True)
        np.testing.assert_allclose(s[name + '_mean'], a[1:n - 1].astype(F64).mean(), rtol=1e-12)
        assert f'{s[name + "_mean"]:.4f}' in lines[1]
    print(f"accel error {s['accel_err_mm_raw_mean']:.4f} -> {s['accel_err_mm_smooth_mean']:.4f} mm/frame^2")
    assert s['accel_err_mm_smooth_mean'] < s['accel_err_mm_raw_mean']
    for k in plain:                                                                 # every other array keeps its contents
        if k != 'meta':
            assert np.array_equal(plain[k], out[k], equal_nan=True), k
    assert {k: v for k, v in s.items() if not k.startswith('accel')} == plain['meta']['smooth']
