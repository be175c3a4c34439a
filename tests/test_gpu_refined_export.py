"""The refined-pose export on the GPU (pytest -m gpu): jrr_rotmat_to_axis_angle and jrr_pose_export against the float64 evaluation of
the host restatement (tests/refined_cases.py), `--save_refined` / `--init_refined` through the driver on synthetic batches and on a
dataset directory, and two gloo ranks against one.

Bounds: there is no reference implementation of the log map, so every bound is `3 x (distance of the restatement's float32 evaluation
from its float64 evaluation on THIS test's inputs) + 1e-7` (refined_cases.bound); tests/test_refined_export.py keeps those
distances at or below 1e-6.  Within 1e-3 of pi the rotations are compared as matrices.

Shapes: n = 24 * 5 (less than one workgroup of k_rotmat_log), n = 24 * 43 + 7 (several workgroups, ragged tail); B = 19 poses (three
workgroups of k_pose_export, the last one with three of its eight poses) into a 64-row table.
"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import refined_cases as rc
from conftest import PKG_NAME, ROOT

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
F = np.float32
ULP_PI = float(np.spacing(F(np.pi)))


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


# ---- 1. the log map ----
def _device_matrices(n, seed):
    """the cases as the library itself makes matrices: planted rows exact, the near-pi and small angles through rodrigues_forward, the
    rest through rot6d_forward of scaled, perturbed columns"""
    eng = _mod('engine')
    m = n - rc.N_PLANTED
    special = 2 * (m // 4)
    aa = rc.axis_angle_cases(n, seed)
    R = torch.empty(n, 3, 3, device=DEV)
    R[:rc.N_PLANTED] = T(rc.planted_matrices()).to(DEV)
    a, b = rc.N_PLANTED, rc.N_PLANTED + special
    R[a:b] = eng.rodrigues_forward(T(aa[a:b].astype(F)).to(DEV))
    R[b:] = eng.rot6d_forward(T(rc.rot6d_cases(n, seed)[b:]).to(DEV))
    return R.contiguous()


@pytest.mark.parametrize('n,seed', [(24 * 5, 21), (24 * 43 + 7, 22)])
def test_rotmat_to_axis_angle_against_float64(n, seed):
    eng, utils = _mod('engine'), _mod('utils')
    R = _device_matrices(n, seed)
    R32 = R.cpu().numpy()
    aa64, d_vec, d_mat, d_rt = rc.yardsticks(R32)
    buf = torch.full((n * 3 + 32,), 7.0, device=DEV)                     # guard floats on either side of the output
    got_dev = eng.rotmat_to_axis_angle(R)
    lib_mod = _mod('_lib')
    out = buf[16:16 + n * 3].view(n, 3)
    lib_mod.check(lib_mod.load().jrr_rotmat_to_axis_angle(lib_mod.ptr(R), lib_mod.ptr(out), n, lib_mod.stream_ptr(R.device)), 'log')
    torch.cuda.synchronize()
    assert (buf[:16] == 7.0).all().item() and (buf[-16:] == 7.0).all().item() and torch.equal(out, got_dev)
    got = got_dev.cpu().numpy()
    g_vec, g_mat = rc.distances(got, aa64)
    back = eng.rodrigues_forward(got_dev)
    g_rt = float((back - R).abs().max().item())
    ang = np.linalg.norm(got.astype(np.float64), axis=1)
    near = int((np.linalg.norm(aa64, axis=1) >= np.pi - rc.NEAR_PI).sum())
    print(f'n={n}: aa {g_vec:.3e} (yardstick {d_vec:.3e}, bound {rc.bound(d_vec):.3e})  matrix {g_mat:.3e} ({d_mat:.3e}, {rc.bound(d_mat):.3e})  '
          f'round trip {g_rt:.3e} ({d_rt:.3e}, {rc.bound(d_rt):.3e})  largest angle pi32 {(ang.max() - float(F(np.pi))) / ULP_PI:+.2f} ulp  '
          f'{near} rows within 1e-3 of pi')
    assert near >= rc.N_PLANTED - 1
    assert g_vec <= rc.bound(d_vec)
    assert g_mat <= rc.bound(d_mat)
    assert g_rt <= rc.bound(d_rt)
    assert ang.max() <= float(F(np.pi)) + ULP_PI                        # every angle <= pi (+ 1 ulp)
    assert (got[0] == 0).all()                                           # the exact identity
    pi = float(F(np.pi))
    assert got[1].tolist() == [pi, 0, 0] and got[2].tolist() == [0, pi, 0] and got[3].tolist() == [0, 0, pi]
    assert np.abs(got[1:rc.N_PLANTED] - rc.half_turn_expected()).max() <= 2 * ULP_PI
    assert got[6, 0] > 0 > got[6, 1] and got[6, 2] == 0 and got[4, 2] == 0
    assert torch.equal(utils.rotmat_to_axis_angle(R.view(-1, 1, 3, 3)), got_dev)
    # one NaN matrix in the middle: a NaN vector there, the neighbours to the bit
    Rn = R.clone()
    Rn[n // 2] = float('nan')
    gn = eng.rotmat_to_axis_angle(Rn).cpu().numpy()
    assert np.isnan(gn[n // 2]).all()
    assert np.array_equal(np.delete(gn, n // 2, 0), np.delete(got, n // 2, 0))


def test_rot6d_to_axis_angle_end_to_end():
    utils = _mod('utils')
    n = 24 * 43 + 7
    x = rc.rot6d_cases(n, 23)
    aa64, d_vec, d_mat = rc.yardsticks_6d(x)
    xd = T(x).to(DEV).requires_grad_(True)
    got = utils.rot6d_to_axis_angle(xd.view(n, 6))
    assert not got.requires_grad and got.shape == (n, 3)
    g_vec, g_mat = rc.distances(got.cpu().numpy(), aa64)
    print(f'6-D -> aa, n={n}: aa {g_vec:.3e} (yardstick {d_vec:.3e})  matrix {g_mat:.3e} ({d_mat:.3e})')
    assert g_vec <= rc.bound(d_vec) and g_mat <= rc.bound(d_mat)


# ---- 2. the export ----
B_EX, N_ROWS = 19, 64


def _export(x6d, betas, cam, index, extra, table, status):
    dev = lambda a: None if a is None else T(np.ascontiguousarray(a)).to(DEV)
    _mod('engine').pose_export(dev(x6d), dev(betas), dev(cam), dev(np.asarray(index, dtype=np.int64)), table, status, extra=dev(extra))
    torch.cuda.synchronize()


def _fresh_table():
    buf = torch.zeros(N_ROWS + 2, 240, device=DEV)
    buf[0], buf[-1] = 5.0, 5.0                                           # a guard row on either side
    return buf, buf[1:-1], torch.zeros(1, dtype=torch.int32, device=DEV)


def _check_rows(table, rows_at, x6d, betas, cam, extra):
    """written rows: columns 72-239 to the bit, 0-71 within the end-to-end bound; every other row zero"""
    host = table.cpu().numpy()
    want = rc.host_rows(x6d, betas, cam, extra)
    rows_at = np.asarray(rows_at)
    assert np.array_equal(host[rows_at][:, 72:], want[:, 72:], equal_nan=True)
    aa64, d_vec, d_mat = rc.yardsticks_6d(x6d.reshape(-1, 6))
    g_vec, g_mat = rc.distances(host[rows_at][:, :72].reshape(-1, 3), aa64)
    assert g_vec <= rc.bound(d_vec) and g_mat <= rc.bound(d_mat), (g_vec, d_vec, g_mat, d_mat)
    rest = np.setdiff1d(np.arange(N_ROWS), rows_at)
    assert not host[rest].any()
    return g_vec, d_vec, g_mat, d_mat


@pytest.mark.parametrize('n_extra', [3, 0])
def test_pose_export_rows_status_and_guards(n_extra):
    x6d, betas, cam = rc.export_case(B_EX, 31)
    rng = np.random.RandomState(32)
    index = rng.permutation(N_ROWS)[:B_EX]
    extra = rng.normal(size=(B_EX, n_extra)).astype(F) if n_extra else None     # None: extra = NULL
    buf, table, status = _fresh_table()
    _export(x6d, betas, cam, index, extra, table, status)
    print('B=19 n_extra=%d: aa %.3e (yardstick %.3e)  matrix %.3e (%.3e)' % ((n_extra,) + _check_rows(table, index, x6d, betas, cam, extra)))
    assert int(status.item()) == 0
    assert (buf[0] == 5.0).all().item() and (buf[-1] == 5.0).all().item()
    assert (table[T(index).to(DEV), 229] == 1.0).all().item() and int((table[:, 229] != 0).sum().item()) == B_EX
    # one index = n_rows and one negative: bit 0 only, those two poses are not stored, everything else is
    buf2, table2, status2 = _fresh_table()
    bad = index.copy()
    bad[3], bad[11] = N_ROWS, -1
    _export(x6d, betas, cam, bad, extra, table2, status2)
    assert int(status2.item()) == 1
    keep = np.setdiff1d(np.arange(B_EX), [3, 11])
    _check_rows(table2, index[keep], x6d[keep], betas[keep], cam[keep], None if extra is None else extra[keep])
    assert (buf2[0] == 5.0).all().item() and (buf2[-1] == 5.0).all().item()
    # an index written before: bit 1, the row is overwritten; a free row beside it is simply written
    free = int(np.setdiff1d(np.arange(N_ROWS), index)[0])
    x2, b2, c2 = rc.export_case(2, 33)
    status.zero_()
    _export(x2, b2, c2, [int(index[5]), free], None, table, status)
    assert int(status.item()) == 2
    host = table.cpu().numpy()
    assert np.array_equal(host[[int(index[5]), free]][:, 72:], rc.host_rows(x2, b2, c2)[:, 72:])
    others = np.delete(np.arange(B_EX), 5)
    assert np.array_equal(host[index[others]][:, 72:], rc.host_rows(x6d, betas, cam, extra)[others][:, 72:])
    # the same index twice in ONE launch is seen as well
    _, table3, status3 = _fresh_table()
    _export(x2, b2, c2, [7, 7], None, table3, status3)
    assert int(status3.item()) == 2 and int((table3[:, 229] != 0).sum().item()) == 1


def test_refined_table_add_and_finish_on_the_device(tmp_path):
    refined = _mod('refined')
    x6d, betas, cam = rc.export_case(B_EX, 41)
    index = np.random.RandomState(42).permutation(N_ROWS)[:B_EX]
    t = refined.RefinedTable(N_ROWS, DEV)
    err = torch.rand(B_EX, device=DEV)
    t.add(T(index).to(DEV), T(x6d).to(DEV), T(betas).to(DEV), T(cam).to(DEV), {'joint_err_m': err, 'iou_after': torch.rand(B_EX, device=DEV).double()})
    arr = t.finish(str(tmp_path / 'r'), {'inner_iters': 0})
    assert arr['has_refined'].sum() == B_EX and arr['has_refined'][index].all()
    assert np.array_equal(arr['pose6d'][index], x6d) and np.array_equal(arr['shape'][index], betas) and np.array_equal(arr['cam'][index], cam)
    assert np.array_equal(arr['joint_err_m'][index], err.cpu().numpy()) and np.array_equal(arr['mpjpe_mm'][index], err.cpu().numpy() * F(1000))
    assert np.isnan(arr['joint_sqerr'][index]).all() and np.isfinite(arr['iou_after'][index]).all()
    back = refined.load(str(tmp_path / 'r'), n=N_ROWS)
    assert np.array_equal(back['pose'], arr['pose']) and back['meta']['refined'] == B_EX
    with pytest.raises(ValueError, match='on cuda:0'):                   # add() copies nothing from the host
        t.add(T(index[:1]), T(x6d[:1]).to(DEV), T(betas[:1]).to(DEV), T(cam[:1]).to(DEV))
    t.add(T(index[:1]).to(DEV), T(x6d[:1]).to(DEV), T(betas[:1]).to(DEV), T(cam[:1]).to(DEV))          # a second visit of a sample
    with pytest.raises(RuntimeError, match='bit 1'):
        t.finish(str(tmp_path / 'twice'))


# ---- 3. the driver ----
SYN_FLAGS = ['--batch_size', '24', '--synthetic_batches', '2', '--inner_iters', '3', '--synthetic', '--device', DEV]


def _driver(flags):
    argsmod = _mod('args')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(flags + ['--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent'])
    try:
        torch.manual_seed(0)
        return _mod('optimize').optimize_pose_refiner(log=lambda r: None)
    finally:
        argsmod._LazyArgs._ns = saved


def _round_trip_check(arr, rows):
    """`pose` through batch_rodrigues gives the matrices of `pose6d`, within the round-trip bound of those matrices"""
    eng = _mod('engine')
    R = eng.rot6d_forward(T(arr['pose6d'][rows]).to(DEV).reshape(-1, 6))
    d_rt = rc.yardsticks(R.cpu().numpy())[3]
    g_rt = float((eng.rodrigues_forward(T(arr['pose'][rows]).to(DEV).reshape(-1, 3)) - R).abs().max().item())
    print(f'pose -> R against rot6d_forward(pose6d): {g_rt:.3e} (yardstick {d_rt:.3e}, bound {rc.bound(d_rt):.3e})')
    assert g_rt <= rc.bound(d_rt)


def test_driver_save_refined_on_synthetic_batches(tmp_path):
    refined = _mod('refined')
    out_dir = str(tmp_path / 'refined')
    res = _driver(SYN_FLAGS + ['--save_refined', out_dir])
    plain = _driver(SYN_FLAGS)
    # the refinement itself is the same to the bit, and so is the record apart from its timings
    for k in ('x6d', 'betas', 'cam', 'J_regressor', 'disc_flat', 'sdisc_flat'):
        assert torch.equal(res[k], plain[k]), k
    timings = ('seconds', 'seconds_batch')
    assert len(res['history']) == len(plain['history']) == 2
    for a, b in zip(res['history'], plain['history']):
        assert {k: v for k, v in a.items() if k not in timings} == {k: v for k, v in b.items() if k not in timings}
    assert 'index' not in plain and res['index'] is None
    arr = refined.load(out_dir, n=48)
    assert arr['has_refined'].tolist() == [1] * 48
    assert np.array_equal(arr['pose6d'][24:], res['x6d'].cpu().numpy()) and np.array_equal(arr['shape'][24:], res['betas'].cpu().numpy())
    assert np.array_equal(arr['cam'][24:], res['cam'].cpu().numpy())
    _round_trip_check(arr, np.arange(48))
    for it, rec in enumerate(res['history']):
        rows = slice(24 * it, 24 * it + 24)
        print(f"batch {it}: mean mpjpe_mm {arr['mpjpe_mm'][rows].mean()!r} record {rec['mpjpe'] + rec['mpjpe difference']!r}")
        np.testing.assert_allclose(arr['mpjpe_mm'][rows].astype(np.float64).mean(), rec['mpjpe'] + rec['mpjpe difference'], rtol=1e-5)
        np.testing.assert_allclose(arr['pampjpe_mm'][rows].astype(np.float64).mean(), rec['pampjpe'] + rec['pampjpe difference'], rtol=1e-5)
        np.testing.assert_allclose(arr['joint_sqerr'][rows].astype(np.float64).sum() / (24 * 51), rec['joint_loss'], rtol=1e-5)
    assert np.isfinite(arr['pose_disc_sq']).all() and np.isnan(arr['shape_disc_sq']).all() and np.isnan(arr['iou_after']).all()
    meta = arr['meta']
    assert meta['inner_iters'] == 3 and meta['n'] == 48 and meta['refined'] == 48 and meta['layout_version'] == 1
    assert meta['flags']['batch_size'] == 24 and meta['flags']['save_refined'] == out_dir and len(meta['j_regressor_sha256_16']) == 16
    assert meta['body_model'] == res['history'][0]['body_model']


def test_driver_on_a_dataset_then_init_refined(smpl_model_np, j_h36m_np, tmp_path):
    """40 samples, batches of 24: a shuffled loader and a ragged second batch of 16"""
    import oracle
    sm, refined = _mod('smpl_model'), _mod('refined')
    n = 40
    rng = np.random.RandomState(3)
    aa = rng.normal(0, 0.3, size=(n, 24, 3)).astype(F)
    full = sm.synthetic_batch(smpl_model_np, j_h36m_np, n, seed=0)
    d = tmp_path / 'precomputed_val'
    d.mkdir()
    tensors = {'bboxes': torch.tensor([[100., 200., 700., 800.]]).repeat(n, 1), 'betas': T(full['betas']),
               'estimated_translation': T(full['cam']), 'gt_j2d': torch.rand(n, 17, 2) * 1000, 'gt_j3d': T(full['gt_j3d']),
               'intrinsics': torch.eye(3).repeat(n, 1, 1), 'orient': T(aa[:, 0]), 'pose': T(aa[:, 1:].reshape(n, 69))}
    for k, v in tensors.items():
        torch.save(v, str(d / f'{k}.pt'))
    flags = ['--batch_size', '24', '--inner_iters', '2', '--device', DEV, '--synthetic', '--data_root', str(tmp_path)]
    out_dir = str(tmp_path / 'refined')
    res = _driver(flags + ['--save_refined', out_dir])
    plain = _driver(flags)
    for k in ('x6d', 'betas', 'cam', 'J_regressor'):
        assert torch.equal(res[k], plain[k]), k
    assert len(res['history']) == 2 and res['x6d'].shape[0] == 16
    arr = refined.load(out_dir, n=n)
    assert arr['has_refined'].tolist() == [1] * n                       # every sample once: finish() raises on a second visit
    # rows sit at their dataset indices: the camera translation is not optimised by these flags, the start pose is the dataset's
    assert np.array_equal(arr['cam'], full['cam'])
    start = oracle.rodrigues(T(aa).reshape(-1, 3)).view(n, 24, 3, 3)[..., :, :2].reshape(n, 24, 6).numpy()
    assert np.abs(arr['pose6d'] - start).max() < 0.1 and np.abs(arr['pose6d'] - start).max() > 1e-4
    idx = res['index'].numpy()
    assert idx.shape == (16,) and len(set(idx.tolist())) == 16
    assert np.array_equal(arr['pose6d'][idx], res['x6d'].cpu().numpy()) and np.array_equal(arr['shape'][idx], res['betas'].cpu().numpy())
    _round_trip_check(arr, np.arange(n))
    # a second pass starts from the bits the first one ended with
    again = _driver(flags[:2] + ['--inner_iters', '0'] + flags[4:] + ['--init_refined', out_dir])
    idx2 = again['index'].numpy()
    assert np.array_equal(idx2, idx)                                    # the same seed shuffles the same way
    assert np.array_equal(again['x6d'].cpu().numpy(), arr['pose6d'][idx2]) and np.array_equal(again['betas'].cpu().numpy(), arr['shape'][idx2])
    assert np.array_equal(again['cam'].cpu().numpy(), arr['cam'][idx2])


# ---- 4. two gloo ranks on one GPU ----
@pytest.fixture(scope='module')
def rank_runs(tmp_path_factory):
    """the driver in rank processes of their own (tests/dp_worker.py): one rank, and two ranks over gloo sharing cuda:0"""
    tmp = str(tmp_path_factory.mktemp('refined_dp'))
    worker = os.path.join(ROOT, 'tests', 'dp_worker.py')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmds = {
        'w1': [sys.executable, worker, os.path.join(tmp, 'w1')] + SYN_FLAGS + ['--save_refined', os.path.join(tmp, 'ref1')],
        'w2': [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
               '--master-port', '29573', worker, os.path.join(tmp, 'w2')] + SYN_FLAGS
              + ['--single_device', '--dist_backend', 'gloo', '--save_refined', os.path.join(tmp, 'ref2')],
    }
    procs = {k: subprocess.Popen(c, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for k, c in cmds.items()}
    outs = {}
    for k, p in procs.items():
        try:
            outs[k] = (p.communicate(timeout=600)[0], p.returncode)
        except subprocess.TimeoutExpired:
            p.kill()
            outs[k] = (p.communicate()[0], -999)
    for k, (text, rc_) in outs.items():
        assert rc_ == 0, f'{k} failed (rc {rc_}):\n{text[-3000:]}'
    return tmp


def test_two_ranks_save_what_one_rank_saves(rank_runs):
    refined = _mod('refined')
    one, two = refined.load(os.path.join(rank_runs, 'ref1'), n=48), refined.load(os.path.join(rank_runs, 'ref2'), n=48)
    assert sorted(os.listdir(os.path.join(rank_runs, 'ref2'))) == ['meta.json', 'refined.npz']
    assert np.array_equal(one['has_refined'], two['has_refined']) and one['has_refined'].all()
    d6, ds = np.abs(one['pose6d'] - two['pose6d']).max(), np.abs(one['shape'] - two['shape']).max()
    print(f'two ranks against one: pose6d {d6:.3e}  shape {ds:.3e}')
    assert d6 <= 2e-4 and ds <= 2e-4
    # each rank's shard of the last batch sits where the single process put those poses
    for r, (lo, hi) in enumerate([(0, 12), (12, 24)]):
        w = dict(np.load(os.path.join(rank_runs, f'w2.rank{r}.npz')))
        assert (int(w['lo']), int(w['hi'])) == (lo, hi)
        assert np.array_equal(two['pose6d'][24 + lo:24 + hi], w['x6d']) and np.array_equal(two['shape'][24 + lo:24 + hi], w['betas'])
    h = json.loads(str(np.load(os.path.join(rank_runs, 'w1.rank0.npz'))['history']))
    np.testing.assert_allclose(one['mpjpe_mm'][:24].astype(np.float64).mean(), h[0]['mpjpe'] + h[0]['mpjpe difference'], rtol=1e-5)
