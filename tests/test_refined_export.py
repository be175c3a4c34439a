"""The refined-pose export without a GPU: the float32 restatement of the log map against its float64 evaluation (the yardsticks
the GPU tests scale), the canonical form, the C ABI rows, RefinedTable.finish / load on CPU tensors (one process and two gloo
ranks), every error case, and the `--init_refined` overlay of the dataset loader."""
import importlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import refined_cases as rc
from conftest import PKG_NAME, ROOT

F = np.float32
T = torch.from_numpy


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


# ---- 1. the yardsticks ----
@pytest.mark.parametrize('n,seed', [(24 * 5, 11), (24 * 43 + 7, 12), (20000, 13)])
def test_float32_restatement_stays_within_1e6_of_float64(n, seed):
    R = rc.matrix_cases(n, seed)
    aa64, d_vec, d_mat, d_rt = rc.yardsticks(R)
    _, d6_vec, d6_mat = rc.yardsticks_6d(rc.rot6d_cases(n, seed))
    print(f'n={n}: aa {d_vec:.3e}  matrix {d_mat:.3e}  round trip {d_rt:.3e}  from 6-D: aa {d6_vec:.3e} matrix {d6_mat:.3e}')
    for d in (d_vec, d_mat, d_rt, d6_vec, d6_mat):
        assert d <= 1e-6
    ang = np.linalg.norm(aa64, axis=1)
    assert ang.max() <= np.pi + 1e-15 and (ang > np.pi - rc.NEAR_PI).sum() >= rc.N_PLANTED - 1       # the near-pi rows are there
    ang32 = np.linalg.norm(rc.log_map(R, F).astype(np.float64), axis=1)
    assert ang32.max() <= float(F(np.pi)) + float(np.spacing(F(np.pi)))
    # small angles: the error is relative (a few ulp of an angle below 1e-2 is below 1e-8)
    small = (ang < 1e-2) & (ang > 0)
    assert small.sum() >= n // 8
    d_small = np.abs(rc.log_map(R[small], F) - aa64[small]).max()
    print(f'      angles below 1e-2: {d_small:.3e}')
    assert d_small <= 1e-8


def test_textbook_inverse_is_useless_near_pi():
    """why the kernel is not acos((tr - 1) / 2) with the axis from the antisymmetric part: in float32 that loses the whole matrix"""
    R = rc.matrix_cases(2000, 5)
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    with np.errstate(all='ignore'):
        th = np.arccos(np.clip((tr - F(1)) / F(2), F(-1), F(1)))
        v = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], 1) / (F(2) * np.sin(th))[:, None]
        back = rc.rodrigues(np.nan_to_num(v * th[:, None]), np.float64, quirk=False)
    assert np.abs(back - R).max() > 0.5
    assert rc.yardsticks(R)[3] <= 1e-6


# ---- 2. the canonical form ----
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_canonical_vectors_of_the_planted_rotations(dtype):
    aa = rc.log_map(rc.planted_matrices(), dtype)
    assert (aa[0] == 0).all()                                                   # the exact identity: exactly zero
    pi = dtype(np.pi)
    assert aa[1].tolist() == [pi, 0, 0] and aa[2].tolist() == [0, pi, 0] and aa[3].tolist() == [0, 0, pi]      # diag(-1,-1,1) -> (0,0,pi)
    want = rc.half_turn_expected()
    assert np.abs(aa[1:] - want).max() <= 2 * np.spacing(F(np.pi))
    assert aa[4, 2] == 0 and aa[6, 2] == 0 and aa[6, 0] > 0 > aa[6, 1]          # (-1,2,0)/sqrt 5 -> (+1.405, -2.810, 0)
    assert abs(aa[6, 0] - 1.405) < 1e-3 and abs(aa[6, 1] + 2.810) < 1e-3
    # either sign of the same half-turn matrix input gives the one answer; just below pi both signs survive
    n = rc.HALF_TURN_AXES[5] / np.linalg.norm(rc.HALF_TURN_AXES[5])
    for sign in (1.0, -1.0):
        R = rc.rodrigues((sign * (np.pi - 1e-3) * n)[None], np.float64, quirk=False)
        got = rc.log_map(R, dtype)[0]
        assert np.abs(got - sign * (np.pi - 1e-3) * n).max() < 1e-5


def test_non_finite_input_stays_in_its_row():
    R = rc.matrix_cases(40, 3)
    clean = rc.log_map(R, F)
    for bad in (np.nan, np.inf):
        Rb = R.copy()
        Rb[17] = bad
        got = rc.log_map(Rb, F)
        assert not np.isfinite(got[17]).any()
        assert np.array_equal(np.delete(got, 17, 0), np.delete(clean, 17, 0))


# ---- 3. the C ABI ----
def test_export_symbols_declared_exported_and_in_the_table():
    hdr = open(os.path.join(ROOT, 'include', 'jrr.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    lib_mod, refined = _mod('_lib'), _mod('refined')
    _mod('build').build(verbose=False)
    lib = lib_mod.load()
    for name in ('jrr_rotmat_to_axis_angle', 'jrr_pose_export'):
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in lib_mod.SIGNATURES and hasattr(lib, name), name
        assert re.search(r'\|[^|\n]*`' + name + r'`[^|\n]*\|', doc), name
    assert 'export.hip' in _mod('build').SOURCES
    # the header states the canonical form and what the map inverts
    assert '[0, pi]' in hdr and 'first non-zero component' in hdr and 'jrr_rodrigues_forward up to that' in hdr.replace('\n * ', ' ') and '+1e-8' in hdr
    # one layout, stated twice
    consts = {k: int(v) for k, v in re.findall(r'\b(JRR_EXPORT_[A-Z0-9_]+) = (\d+)', hdr)}
    assert consts == {'JRR_EXPORT_LAYOUT_VERSION': refined.LAYOUT_VERSION, 'JRR_EXPORT_ROW': refined.ROW,
                      'JRR_EXPORT_POSE': refined.POSE, 'JRR_EXPORT_POSE6D': refined.POSE6D, 'JRR_EXPORT_BETAS': refined.BETAS,
                      'JRR_EXPORT_CAM': refined.CAM, 'JRR_EXPORT_MARKER': refined.MARKER, 'JRR_EXPORT_EXTRA': refined.EXTRA,
                      'JRR_EXPORT_MAX_EXTRA': refined.MAX_EXTRA, 'JRR_EXPORT_STATUS_INDEX': 1, 'JRR_EXPORT_STATUS_TWICE': 2}
    assert (refined.POSE, refined.POSE6D, refined.BETAS, refined.CAM, refined.MARKER, refined.EXTRA) == (0, 72, 216, 226, 229, 230)
    assert len(refined.EXTRA_NAMES) <= refined.MAX_EXTRA
    # argument errors come back as a status, nothing is launched (the pointers are never read)
    import ctypes
    p = ctypes.c_void_p(4096)
    ok = lambda **kw: lib.jrr_pose_export(*[kw.get(k, d) for k, d in (('x', p), ('b', p), ('c', p), ('e', p), ('ne', 3), ('i', p), ('t', p), ('n', 64),
                                                                       ('s', p), ('B', 0), ('st', None))])
    assert ok() == 0                                                                        # an empty batch launches nothing
    assert ok(ne=11) == -1 and b'n_extra 11' in lib.jrr_last_error()
    assert ok(ne=-1) == -1
    assert ok(e=None, ne=0) == 0
    for k in ('x', 'b', 'c', 'i', 't', 's'):
        assert ok(**{k: None}) == -1, k
    assert ok(t=ctypes.c_void_p(4096 + 8)) == -1 and b'16-byte aligned' in lib.jrr_last_error()
    assert ok(n=-1) == -1 and ok(B=-1) == -1
    assert lib.jrr_rotmat_to_axis_angle(p, p, 0, None) == 0
    assert lib.jrr_rotmat_to_axis_angle(None, p, 4, None) == -1 and lib.jrr_rotmat_to_axis_angle(p, None, 4, None) == -1
    assert lib.jrr_rotmat_to_axis_angle(p, p, -1, None) == -1


def test_flags_default_to_off_and_init_needs_a_dataset():
    a, opt = _mod('args'), _mod('optimize')
    ns = a.get_args([])
    assert ns.save_refined is None and ns.init_refined is None
    ns = a.get_args(['--save_refined', 'out', '--init_refined', 'in'])
    assert ns.save_refined == 'out' and ns.init_refined == 'in'
    for k, v in a.REFERENCE_FLAGS.items():
        assert getattr(ns, k) == v, k
    saved = a._LazyArgs._ns
    try:
        a._LazyArgs._ns = a.get_args(['--init_refined', 'somewhere', '--synthetic'])
        with pytest.raises(ValueError, match='--init_refined needs --data_root'):
            opt.optimize_pose_refiner(log=lambda r: None)
    finally:
        a._LazyArgs._ns = saved


# ---- 4. the table on CPU tensors ----
def _filled(n_rows, rows_at, seed, extra_cols=7):
    """a CPU RefinedTable whose rows `rows_at` hold the host restatement's records; (table, the arrays one expects)"""
    refined = _mod('refined')
    B = len(rows_at)
    x6d, betas, cam = rc.export_case(B, seed)
    extra = np.random.RandomState(seed + 9).uniform(size=(B, extra_cols)).astype(F)
    extra[:, 3] = np.nan                                                          # a metric the run did not compute
    rows = rc.host_rows(x6d, betas, cam, extra)
    t = refined.RefinedTable(n_rows, 'cpu')
    t.table[torch.as_tensor(rows_at)] = T(rows)
    return t, rows


def _check_arrays(arr, n_rows, rows_at, rows):
    refined = _mod('refined')
    has = np.zeros(n_rows, dtype=np.uint8)
    has[rows_at] = 1
    assert arr['has_refined'].dtype == np.uint8 and np.array_equal(arr['has_refined'], has)
    full = np.zeros((n_rows, 240), dtype=F)
    full[rows_at] = rows
    assert np.array_equal(arr['pose'], full[:, :72]) and np.array_equal(arr['pose6d'], full[:, 72:216].reshape(n_rows, 24, 6))
    assert np.array_equal(arr['shape'], full[:, 216:226]) and np.array_equal(arr['cam'], full[:, 226:229])
    for k, name in enumerate(refined.EXTRA_NAMES):
        assert np.array_equal(arr[name], full[:, 230 + k], equal_nan=True), name
    assert np.isnan(arr['pose_disc_sq'][rows_at]).all()
    assert np.array_equal(arr['mpjpe_mm'], full[:, 230] * F(1000)) and np.array_equal(arr['pampjpe_mm'], full[:, 231] * F(1000))
    for k in ('pose', 'pose6d', 'shape', 'cam', 'mpjpe_mm') + tuple(refined.EXTRA_NAMES):
        assert arr[k].dtype == np.float32, k


def test_finish_and_load_in_one_process(tmp_path):
    refined = _mod('refined')
    rows_at = [5, 0, 11, 7, 3]
    t, rows = _filled(12, rows_at, seed=2)
    out = str(tmp_path / 'ref')
    arr = t.finish(out, {'flags': {'batch_size': 5}, 'body_model': 'synthetic', 'j_regressor_sha256_16': '0' * 16, 'inner_iters': 3})
    _check_arrays(arr, 12, rows_at, rows)
    assert sorted(os.listdir(out)) == ['meta.json', 'refined.npz']
    back = refined.load(out, n=12)
    meta = back.pop('meta')
    assert set(back) == set(arr) and all(np.array_equal(back[k], arr[k], equal_nan=True) for k in arr)
    assert meta['layout_version'] == refined.LAYOUT_VERSION == 1 and meta['n'] == 12 and meta['refined'] == 5
    assert meta['inner_iters'] == 3 and meta['body_model'] == 'synthetic' and meta['flags'] == {'batch_size': 5}
    assert meta['extra_names'] == list(refined.EXTRA_NAMES)
    with np.load(os.path.join(out, 'refined.npz'), allow_pickle=False) as z:       # plain numpy, no pickle
        assert set(z.files) == set(arr)


def test_every_error_case_raises(tmp_path):
    refined = _mod('refined')
    for bit, word in ((1, 'bit 0'), (2, 'bit 1'), (3, 'bit 0')):
        t, _ = _filled(6, [1, 4], seed=3)
        t.status.fill_(bit)
        with pytest.raises(RuntimeError, match=word):
            t.finish(str(tmp_path / f'status{bit}'))
        assert not os.path.exists(str(tmp_path / f'status{bit}'))
    t, _ = _filled(6, [1, 4], seed=3)
    t.table[4, refined.MARKER] = 2.0                                               # two ranks stored the same sample
    with pytest.raises(RuntimeError, match='marker 2.0 in row 4'):
        t.finish(str(tmp_path / 'marker'))
    t, _ = _filled(6, [1, 4], seed=3)
    t.table[2, refined.MARKER] = float('nan')
    with pytest.raises(RuntimeError, match='marker'):
        t.finish(str(tmp_path / 'marker_nan'))
    t, _ = _filled(6, [1, 4], seed=3)
    good = str(tmp_path / 'good')
    t.finish(good)
    with pytest.raises(ValueError, match='holds 6 samples, 7 expected'):
        refined.load(good, n=7)
    meta = json.load(open(os.path.join(good, 'meta.json')))
    meta['layout_version'] = 2
    json.dump(meta, open(os.path.join(good, 'meta.json'), 'w'))
    with pytest.raises(ValueError, match='layout version 2'):
        refined.load(good)
    t, _ = _filled(6, [1, 4], seed=3)
    with pytest.raises(ValueError, match='unknown extras'):
        t.add(torch.zeros(1, dtype=torch.int64), torch.zeros(1, 24, 6), torch.zeros(1, 10), torch.zeros(1, 3), {'iou': None})


_RANK_WORKER = r'''
import importlib, os, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch.distributed as dist
import refined_cases as rc
refined = importlib.import_module("joint-regressor-refinement_amd.refined")
dist.init_process_group("gloo")
rank = dist.get_rank()
rows_at = [int(v) for v in sys.argv[3].split(",")]
B = len(rows_at)
x6d, betas, cam = rc.export_case(B, 2)
extra = np.random.RandomState(11).uniform(size=(B, 7)).astype(np.float32); extra[:, 3] = np.nan
rows = rc.host_rows(x6d, betas, cam, extra)
lo, hi = (0, B // 2) if rank == 0 else (B // 2, B)              # disjoint rows per rank
t = refined.RefinedTable(int(sys.argv[4]), "cpu")
t.table[torch.as_tensor(rows_at[lo:hi])] = torch.from_numpy(rows[lo:hi])
if len(sys.argv) > 5 and rank == 1:
    t.table[rows_at[0]] = torch.from_numpy(rows[0])             # ... or not: rank 1 stores a sample of rank 0 as well
try:
    t.finish(os.path.join(sys.argv[2], "rank%d" % rank), {"inner_iters": 3})
    outcome = "ok"
except RuntimeError as exc:
    outcome = "RuntimeError: %s" % exc
open(os.path.join(sys.argv[2], "outcome%d.txt" % rank), "w").write(outcome)
dist.barrier()
dist.destroy_process_group()
'''


def _two_ranks(tmp_path, out, rows_at, n_rows, port, overlap=False):
    script = tmp_path / 'refined_rank_worker.py'
    script.write_text(_RANK_WORKER)
    os.makedirs(out, exist_ok=True)
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), OMP_NUM_THREADS='2')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1', '--master-port', str(port),
           str(script), ROOT, out, ','.join(str(r) for r in rows_at), str(n_rows)] + (['overlap'] if overlap else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [open(os.path.join(out, f'outcome{k}.txt')).read() for k in (0, 1)]


def test_two_gloo_ranks_write_what_one_process_writes(tmp_path):
    refined = _mod('refined')
    rows_at, n_rows = [5, 0, 11, 7, 3, 9], 12
    t, rows = _filled(n_rows, rows_at, seed=2)                   # the worker below draws the same records
    one = t.finish(str(tmp_path / 'one'), {'inner_iters': 3})
    out = str(tmp_path / 'two')
    assert _two_ranks(tmp_path, out, rows_at, n_rows, 29571) == ['ok', 'ok']
    assert sorted(os.listdir(out)) == ['outcome0.txt', 'outcome1.txt', 'rank0']            # rank 0 alone wrote
    two = refined.load(os.path.join(out, 'rank0'), n=n_rows)
    two.pop('meta')
    _check_arrays(two, n_rows, rows_at, rows)
    assert set(two) == set(one) and all(np.array_equal(two[k], one[k], equal_nan=True) for k in one)
    # a sample stored by both ranks: its marker sums to 2 and every rank raises
    out2 = str(tmp_path / 'overlap')
    outcomes = _two_ranks(tmp_path, out2, rows_at, n_rows, 29572, overlap=True)
    assert all(o.startswith('RuntimeError') and 'marker 2.0 in row 5' in o for o in outcomes), outcomes
    assert sorted(os.listdir(out2)) == ['outcome0.txt', 'outcome1.txt']


# ---- 5. the dataset side ----
def _write_6d_dataset(root, n, seed):
    loc = os.path.join(root, 'precomputed_val')
    os.makedirs(loc)
    g = torch.Generator().manual_seed(seed)
    files = dict(bboxes=torch.tensor([[100., 200., 700., 600.]]).repeat(n, 1), betas=torch.randn(n, 10, generator=g),
                 estimated_translation=torch.randn(n, 3, generator=g), gt_j2d=torch.rand(n, 17, 2, generator=g) * 1000,
                 gt_j3d=torch.randn(n, 17, 3, generator=g) * 300, intrinsics=torch.eye(3).repeat(n, 1, 1),
                 orient=torch.randn(n, 1, 6, generator=g), pose=torch.randn(n, 23, 6, generator=g))
    for k, v in files.items():
        torch.save(v, os.path.join(loc, f'{k}.pt'))
    return files


def test_dataset_index_is_opt_in(tmp_path):
    d = _mod('data')
    _write_6d_dataset(str(tmp_path), 5, 0)
    plain = {'bboxes', 'betas', 'cam', 'gt_j2d', 'gt_j3d', 'intrinsics', 'orient', 'pose', 'inc_gt'}
    assert set(d.data_set('validation', root=str(tmp_path))[3]) == plain
    s = d.data_set('validation', root=str(tmp_path), with_index=True)[3]
    assert set(s) == plain | {'index'} and int(s['index']) == 3 and s['index'].dtype == torch.int64


def test_init_refined_overlays_exactly_the_refined_rows(tmp_path):
    refined, opt = _mod('refined'), _mod('batches')
    n, B = 13, 5
    files = _write_6d_dataset(str(tmp_path), n, 1)
    rows_at = [2, 3, 7, 12]
    t, rows = _filled(n, rows_at, seed=4)
    table_dir = str(tmp_path / 'table')
    t.finish(table_dir)
    init = refined.load(table_dir, n=n)
    seen = np.zeros(n, dtype=int)
    sizes = []
    plain = list(opt.dataset_batches(str(tmp_path), B, 0, 'cpu'))
    for full, ref in zip(opt.dataset_batches(str(tmp_path), B, 0, 'cpu', init_refined=init), plain):
        assert 'index' not in ref and 'n_samples' not in ref and full['n_samples'] == n
        idx = full['index'].numpy()
        sizes.append(len(idx))
        seen[idx] += 1
        for k, i in enumerate(idx):
            if i in rows_at:                                    # the table's bits
                r = rows[rows_at.index(i)]
                assert np.array_equal(full['pose6d'][k].numpy().reshape(-1), r[72:216])
                assert np.array_equal(full['betas'][k].numpy(), r[216:226]) and np.array_equal(full['cam'][k].numpy(), r[226:229])
            else:                                               # the dataset's
                x6 = torch.cat([files['orient'][i], files['pose'][i]], 0)
                assert torch.equal(full['pose6d'][k], x6) and torch.equal(full['betas'][k], files['betas'][i])
                assert torch.equal(full['cam'][k], files['estimated_translation'][i])
        assert torch.equal(full['gt_j3d'], ref['gt_j3d'])       # the same shuffled batch as without the table
    assert sizes == [5, 5, 3] and (seen == 1).all()
    with_index = next(opt.dataset_batches(str(tmp_path), B, 0, 'cpu', with_index=True))
    assert torch.equal(with_index['pose6d'], plain[0]['pose6d']) and with_index['index'].shape == (5,)
    # a table of another length is refused
    t2, _ = _filled(n + 1, rows_at, seed=4)
    t2.finish(str(tmp_path / 'longer'))
    with pytest.raises(ValueError, match='the table holds 14 samples, the dataset 13'):
        next(opt.dataset_batches(str(tmp_path), B, 0, 'cpu', init_refined=refined.load(str(tmp_path / 'longer'))))
