"""Bone length and direction errors on the GPU (pytest -m gpu): jrr_bone_error against the float64 evaluation of the host restatement
(tests/bone_cases.py), jrr_bone_accumulate word for word against the integer accumulation of the rows the kernel wrote, the properties
the header promises, and the two places `--eval_bones` takes effect.

Bounds: there is no reference implementation, so each block of per-pose values is held to `3 x (distance of the restatement's float32
evaluation from its float64 evaluation on THIS test's inputs) + 1e-7` (accel_cases.bound), the maximum over the block's entries; the
two angle blocks get 4 x 2^-23 x pi rad more for the device's atan2f.  `ang_pa` ALONE is left out on the poses of the collinear
families (bone_cases.gpu_pool names them): the rotation about a line is free there, as csrc/evalk.h states; every other value of those
poses is compared.

Shapes: a pool of 257 poses -- eval_report_cases.pose_cases and its flat and collinear families, interleaved so that every wave holds
every shape -- at batches 1, 63, 64, 65 and 257 (one below, at and above a wave and a 256-thread workgroup), written inside frames of
sentinel values.
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

import bone_cases as bc
from conftest import PKG_NAME, ROOT

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
F, F64 = np.float32, np.float64
SENTINEL = -7.0


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(pred, gt):
    """jrr_bone_error on host arrays, written into a frame of sentinels: the (B,98) rows, after checking the frame"""
    B = pred.shape[0]
    frame = torch.full((B + 2, bc.VALS), SENTINEL, device=DEV)
    out = _mod('engine').bone_error(T(np.ascontiguousarray(pred)).to(DEV), T(np.ascontiguousarray(gt)).to(DEV), out=frame[1:B + 1])
    assert out.data_ptr() == frame[1:].data_ptr()
    host = frame.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[B + 1] == SENTINEL).all()
    return host[1:B + 1].copy()


def _table(vals, group, n_groups, acc=None):
    """jrr_bone_accumulate of host rows into a table inside a frame of sentinel words"""
    words = n_groups * bc.ROW + bc.TRAILER
    frame = torch.full((words + 16,), -99, dtype=torch.int64, device=DEV)
    frame[8:8 + words] = 0 if acc is None else T(acc).to(DEV)
    _mod('engine').bone_accumulate(T(np.ascontiguousarray(vals)).to(DEV), None if group is None else T(np.ascontiguousarray(group)).to(DEV), n_groups,
                                   frame[8:8 + words])
    host = frame.cpu().numpy()
    assert (host[:8] == -99).all() and (host[8 + words:] == -99).all()
    return host[8:8 + words].copy()


class Pool:
    """bone_cases.gpu_pool with what the restatement says about it (computed once, never changed)"""

    def __init__(self):
        self.pred, self.gt, self.collinear = bc.gpu_pool()
        self.r64, self.r32 = bc.bones(self.pred, self.gt, F64), bc.bones(self.pred, self.gt, F)
        self.bounds = bc.block_bounds(self.r32, self.r64, rows_pa=~self.collinear)
        self.whole = _run(self.pred, self.gt)


@pytest.fixture(scope='module')
def pool():
    return Pool()


# ---- 1. the per-pose values ----
@pytest.mark.parametrize('B', bc.GPU_BATCHES)
def test_values_against_float64_on_every_pose_and_bits_whatever_the_batch(pool, B):
    got = _run(pool.pred[:B], pool.gt[:B])
    assert got.dtype == F and got.shape == (B, bc.VALS) and np.isfinite(got).all()
    named = np.nonzero(pool.collinear[:B])[0]
    assert B < 6 or (named.size and set((named % 6).tolist()) == {4, 5})               # the poses on which ang_pa is not compared
    for name, _, _ in bc.BLOCKS:
        rows = ~pool.collinear[:B] if name == 'ang_pa' else np.ones(B, bool)
        g, w, r = bc.block(got, name)[rows], bc.block(pool.r64[:B], name)[rows], bc.block(pool.r32[:B], name)[rows]
        d = bc.dist(g, w) if rows.any() else 0.0
        print(f'B {B} {name}: {d:.3e} (bound {pool.bounds[name]:.3e}); bits equal to the float32 restatement: {np.array_equal(_bits(g), _bits(r))}')
        assert d <= pool.bounds[name], name
    assert not got[:, bc.ERR_DIR].any() and not got[:, bc.ERR_LEN].any()                # the pelvis: 0 by definition
    assert np.array_equal(_bits(got), _bits(pool.whole[:B]))                            # the same bits alone and inside the 257


def test_a_pose_keeps_its_bits_at_any_position_and_a_second_call_repeats(pool):
    again = _run(pool.pred, pool.gt)
    assert np.array_equal(_bits(again), _bits(pool.whole))
    perm = np.random.RandomState(3).permutation(bc.GPU_POOL)
    moved = _run(pool.pred[perm], pool.gt[perm])
    assert np.array_equal(_bits(moved), _bits(pool.whole[perm]))
    tail = _run(pool.pred[200:], pool.gt[200:])                                         # 57 poses: another lane, another workgroup
    assert np.array_equal(_bits(tail), _bits(pool.whole[200:]))


# ---- 2. the table ----
@pytest.fixture(scope='module')
def tcase():
    pred, gt, group, special = bc.table_case()
    return pred, gt, group, special, _run(pred, gt)


def test_table_is_exactly_the_integer_accumulation_of_the_rows_the_kernel_wrote(pool, tcase):
    pred, gt, group, special, vals = tcase
    table = _table(vals, group, 3)
    want = bc.as_int64(bc.accumulate(vals, group, 3))
    assert table.dtype == np.int64 and np.array_equal(table, want)
    t = table[:-2].reshape(3, bc.ROW)
    assert table[-2:].tolist() == [2, 1] and not t[1].any()                             # two ignored, one with a group outside; group 1 empty
    assert int(t[:, bc.BAD].sum()) == 3 and int(t[:, bc.COUNT].sum()) == 65 - 3 - 3 and (t[[0, 2], bc.COUNT] > 0).all()
    # the three bad poses: NaN where the definition says, BAD only, and no neighbour disturbed
    clean_pred, clean_gt = bc.erc.family_cases('body', 65, 5)
    clean = _run(clean_pred, clean_gt)
    bad = sorted(special[k] for k in ('nan', 'zero_bone', 'constant_pred'))
    others = np.setdiff1d(np.arange(65), bad)
    assert np.array_equal(_bits(vals[others]), _bits(clean[others]))
    assert np.isnan(vals[special['nan']]).any() and np.isnan(vals[special['constant_pred'], bc.ERR_DIR + 1:bc.ERR_DIR + 17]).all()
    z = vals[special['zero_bone']]
    assert z[bc.LEN_PRED + 4] == 0 and np.isnan(z[bc.ERR_DIR + 5]) and np.isfinite(z[bc.ERR_DIR + 4]) and np.isfinite(z[bc.LEN_GT:bc.LEN_GT + 16]).all()
    assert not vals[special['constant_pred'], bc.LEN_PRED:bc.LEN_PRED + 16].any()
    for k in ('nan', 'zero_bone', 'constant_pred'):
        i = special[k]
        alone = _table(vals[i:i + 1], group[i:i + 1], 3)
        assert int(alone.sum()) == 1 and int(alone[int(group[i]) * bc.ROW + bc.BAD]) == 1, k
    # no groups given: everything in group 0, the trailer empty
    table0 = _table(vals, None, 1)
    assert np.array_equal(table0, bc.as_int64(bc.accumulate(vals, None, 1))) and table0[-2:].tolist() == [0, 0] and int(table0[bc.COUNT]) == 62
    # more than one workgroup, every group in every workgroup: the 257 poses of the pool in 5 groups
    g5 = (np.arange(bc.GPU_POOL) % 5).astype(np.int32)
    big = _table(pool.whole, g5, 5)
    assert np.array_equal(big, bc.as_int64(bc.accumulate(pool.whole, g5, 5))) and int(big[:-2].reshape(5, bc.ROW)[:, bc.COUNT].sum()) == bc.GPU_POOL
    # the derived numbers are the float64 restatement's means, to the bound
    with pytest.raises(RuntimeError, match='1 poses carried a group id outside'):
        _mod('bones_report').derive(table, ['a', 'b', 'c'])
    doc = _mod('bones_report').derive(big, list('abcde'))
    assert abs(doc['all']['mpjpe_true_lengths_mm'] - bc.block(pool.r64, 'e_dir').mean() * 1000) <= 1000 * (pool.bounds['e_dir'] + 2.0 ** -25)
    np.testing.assert_allclose(doc['all']['len_pred_mm'], bc.block(pool.r64, 'len_pred').mean(0) * 1000, rtol=0, atol=1000 * (pool.bounds['len_pred'] + 2.0 ** -25))


def test_two_halves_sum_to_the_whole_and_a_permutation_gives_the_same_table(tcase):
    pred, gt, group, special, vals = tcase
    table = _table(vals, group, 3)
    first = _table(vals[:30], group[:30], 3)
    assert first.any() and np.array_equal(_table(vals[30:], group[30:], 3, acc=first), table)
    assert np.array_equal(first + _table(vals[30:], group[30:], 3), table)
    perm = np.random.RandomState(1).permutation(65)
    assert np.array_equal(_table(vals[perm], group[perm], 3), table)


# ---- 3. the two places of --eval_bones ----
def _with_args(flags, fn):
    argsmod = _mod('args')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(flags + ['--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent', '--synthetic', '--device', DEV])
    try:
        torch.manual_seed(0)
        return fn()
    finally:
        argsmod._LazyArgs._ns = saved


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


def test_eval_bones_through_test_pose_refiner_model(tmp_path, smpl_model_np, j_h36m_np, monkeypatch):
    """a 40-sample dataset directory of two subjects with a planted rigid ground truth, batches of 20: bones.json beside an eval.json
    that keeps its bytes, its numbers the float64 restatement's of the same joints"""
    n = 40
    root = str(tmp_path / 'data')
    os.makedirs(root)
    gt, paths = bc.rigid_dataset(n)
    rng = np.random.RandomState(3)
    full = _mod('smpl_model').synthetic_batch(smpl_model_np, j_h36m_np, n, seed=0)
    aa = rng.normal(0, 0.3, size=(n, 24, 3)).astype(F)
    _write_dataset(root, {'bboxes': torch.tensor([[100., 200., 700., 800.]]).repeat(n, 1), 'betas': T(full['betas']),
                          'estimated_translation': T(full['cam']), 'gt_j2d': torch.rand(n, 17, 2) * 1000, 'gt_j3d': T(gt),
                          'intrinsics': torch.eye(3).repeat(n, 1, 1), 'orient': T(aa[:, 0]), 'pose': T(aa[:, 1:].reshape(n, 69))}, paths)
    ck, _, _ = _checkpoint(str(tmp_path))
    evaluation, br = _mod('test'), _mod('bones_report')
    seen = {'before': [], 'after': [], 'gt': []}
    real_add = br.BoneReport.add

    def spy(self, set_name, joints, gt_mm, gid=None, sid=None):                       # the joints the report was fed, for the restatement
        seen[set_name].append(joints.detach().cpu().numpy())
        if set_name == 'before':
            seen['gt'].append(gt_mm.detach().cpu().numpy())
        return real_add(self, set_name, joints, gt_mm, gid, sid)

    flags = ['--batch_size', '20', '--data_root', root, '--eval_j_regressor', ck]
    runs = {}
    for key, extra in (('plain', []), ('bones', ['--eval_bones'])):
        lines = []
        out = str(tmp_path / key)
        if extra:
            monkeypatch.setattr(br.BoneReport, 'add', spy)
        rep = _with_args(flags + ['--eval_report', out] + extra, lambda: evaluation.test_pose_refiner_model(log=lines.append))
        runs[key] = (out, lines, rep)
    (out0, lines0, rep0), (out1, lines1, rep1) = runs['plain'], runs['bones']
    assert sorted(os.listdir(out0)) == ['eval.json', 'eval.md'] and sorted(os.listdir(out1)) == ['bones.json', 'bones.md', 'eval.json', 'eval.md']
    assert open(os.path.join(out0, 'eval.md'), 'rb').read() == open(os.path.join(out1, 'eval.md'), 'rb').read()
    raw0, raw1 = (open(os.path.join(o, 'eval.json'), 'rb').read() for o in (out0, out1))
    assert raw0.replace(out0.encode(), b'DIR') == raw1.replace(out1.encode(), b'DIR')      # byte-identical but for the directory's own name
    assert 'eval_bones' not in json.loads(raw1)['flags']
    assert lines1[:-1] == lines0 and lines1[-1].startswith('bones: before ') and 'bones_report' not in rep0
    doc = br.load(out1)
    assert doc['source'] == 'parameters' and doc['groups'] == ['Eating', 'Walking'] and doc['subjects'] == ['S11', 'S9']
    ev = json.loads(raw1)
    gt_fed = np.concatenate(seen['gt'])
    for which in ('before', 'after'):
        joints = np.concatenate(seen[which])
        assert joints.shape == (n, 17, 3)
        r64, r32 = bc.bones(joints, gt_fed, F64), bc.bones(joints, gt_fed, F)
        b = bc.block_bounds(r32, r64)
        a = doc['sets'][which]['all']
        step = 2.0 ** -25
        assert a['n'] == n and a['n_bad'] == 0 and a['mpjpe_mm'] == ev['regressors'][which]['all']['mpjpe_mm']
        for key, name, unit in (('len_pred_mm', 'len_pred', 1000.0), ('len_gt_mm', 'len_gt', 1000.0), ('ang_deg', 'ang', 180 / np.pi),
                                ('ang_pa_deg', 'ang_pa', 180 / np.pi)):
            d = np.abs(np.asarray(a[key]) - bc.block(r64, name).mean(0) * unit).max()
            print(f'{which} {key}: {d:.3e} (bound {unit * (b[name] + step):.3e})')
            assert d <= unit * (b[name] + step), key
        for key, name in (('mpjpe_true_lengths_mm', 'e_dir'), ('mpjpe_true_directions_mm', 'e_len')):
            d = abs(a[key] - bc.block(r64, name).mean() * 1000)
            print(f'{which} {key}: {a[key]:.4f} mm, {d:.3e} (bound {1000 * (b[name] + step):.3e})')
            assert d <= 1000 * (b[name] + step), key
        assert doc['sets'][which]['groups']['Eating']['n'] == 20 and doc['sets'][which]['groups']['Walking']['mpjpe_mm'] == ev['regressors'][which]['groups']['Walking']['mpjpe_mm']
    rig = doc['rigidity']
    assert rig['mean_gt_mm'] == 0.0 and all(e['gt_mm'] == [0.0] * 16 for e in rig['per_subject'].values())      # the planted skeleton: rigid, exactly
    assert rig['mean_before_mm'] > 0 and rig['mean_after_mm'] > 0 and rig['per_subject']['S9']['n'] == {'before': 20, 'after': 20}
    assert doc['sets']['before']['all']['raw'] != doc['sets']['after']['all']['raw']
    assert doc['sets']['before']['all']['len_gt_mm'] == doc['sets']['after']['all']['len_gt_mm']        # one ground truth


def test_eval_bones_through_eval_vertices_two_gloo_ranks_equal_one(tmp_path, smpl_model_np):
    """40 meshes of two subjects: main.py --eval_vertices under torchrun, two ranks over gloo sharing cuda:0, writes the bones.json bytes
    of one rank"""
    n = 40
    tmp = str(tmp_path)
    ck, J, _ = _checkpoint(tmp)
    _, paths = bc.rigid_dataset(n)
    rng = np.random.RandomState(11)
    verts = (smpl_model_np['v_template'][None] * (1 + 0.1 * rng.rand(n, 1, 1)) + rng.normal(0, 0.002, size=(n, 6890, 3))).astype(F)
    vdir = os.path.join(tmp, 'meshes')
    os.makedirs(vdir)
    np.save(os.path.join(vdir, 'vertices.npy'), verts)
    np.save(os.path.join(vdir, 'gt_j3d.npy'), (np.einsum('jv,nvc->njc', J.astype(F64), verts.astype(F64)) * 1000 + rng.normal(0, 3, size=(n, 17, 3))).astype(F))
    flags = ['--batch_size', '16', '--eval_j_regressor', ck, '--eval_vertices', vdir, '--eval_bones']
    bare = os.path.join(tmp, 'bare')                                                  # no paths.txt: no subjects, and the report says so
    _with_args(flags + ['--eval_report', bare], lambda: _mod('eval_report').evaluate_vertices(log=lambda s: None))
    doc0 = _mod('bones_report').load(bare)
    assert doc0['rigidity'] is None and doc0['groups'] == ['all'] and doc0['sets']['after']['all']['n'] == n
    with open(os.path.join(vdir, 'paths.txt'), 'w') as f:
        f.write('\n'.join(paths) + '\n')
    one = os.path.join(tmp, 'one')
    lines = []
    _with_args(flags + ['--eval_report', one], lambda: _mod('eval_report').evaluate_vertices(log=lines.append))
    assert sorted(os.listdir(one)) == ['bones.json', 'bones.md', 'eval.json', 'eval.md'] and len(lines) == 4 and lines[2].startswith('bones: before ')
    doc = _mod('bones_report').load(one)
    assert doc['source'] == 'vertices' and doc['subjects'] == ['S11', 'S9'] and doc['sets']['before']['all']['n'] == n
    assert doc['rigidity']['per_subject']['S9']['n'] == {'before': 20, 'after': 20} and doc['rigidity']['mean_after_mm'] > 0
    assert doc['sets']['before']['all']['raw'] != doc['sets']['after']['all']['raw']
    two = os.path.join(tmp, 'two')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1', '--master-port', '29592',
           os.path.join(ROOT, 'main.py')] + flags + ['--eval_report', two, '--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent', '--synthetic',
                                                     '--device', DEV, '--single_device', '--dist_backend', 'gloo']
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert sorted(os.listdir(two)) == ['bones.json', 'bones.md', 'eval.json', 'eval.md']
    for name in ('bones.json', 'bones.md'):
        assert open(os.path.join(two, name), 'rb').read() == open(os.path.join(one, name), 'rb').read(), name
