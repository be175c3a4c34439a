"""Bone length and direction errors without a GPU: the host restatement (tests/bone_cases.py) on planted skeletons, `derive` and
`rigidity` on a hand-made table, the flag and what it refuses, the C ABI's argument checks, and bones_report end to end on CPU tensors
with engine.bone_error / engine.bone_accumulate replaced by the restatement (one process and two gloo ranks).

"Exactly" below means bit for bit: the planted inputs are dyadic (bone_cases.dyadic_poses), so every difference and every product of
the definition is exact in float32.  `ang_pa` goes through the FITTED rotation, which is the identity only to rounding even for
identical inputs: it is held to the bound of 0, never to 0 itself."""
import importlib
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import bone_cases as bc
from conftest import PKG_NAME, ROOT

F, F64 = np.float32, np.float64
T = torch.from_numpy


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _both(pred, gt):
    r32, r64 = bc.bones(pred, gt, F), bc.bones(pred, gt, F64)
    return r32, r64, bc.block_bounds(r32, r64)


# ---- 1. the restatement on planted skeletons ----
@pytest.mark.parametrize('dtype', [F, F64])
def test_identical_skeletons_give_exactly_zero(dtype):
    gt, m = bc.dyadic_poses(12)
    r = bc.bones(m.astype(F), gt, dtype)
    assert r.dtype == dtype and r.shape == (12, 98)
    for name in ('ang', 'e_dir', 'e_len'):
        assert not bc.block(r, name).any(), name                                    # 0.0 exactly
    assert np.array_equal(bc.block(r, 'len_pred'), bc.block(r, 'len_gt')) and bc.block(r, 'len_gt').min() > 0      # |delta length| = 0 exactly
    r32, r64, b = _both(m.astype(F), gt)
    print(f'ang_pa of identical skeletons: float32 {bc.block(r32, "ang_pa").max():.3e}, float64 {bc.block(r64, "ang_pa").max():.3e}, bound {b["ang_pa"]:.3e}')
    assert bc.block(r32, 'ang_pa').max() <= b['ang_pa'] and bc.block(r64, 'ang_pa').max() <= 1e-7


def test_a_scaled_skeleton_has_the_directions_and_half_the_length_more():
    gt, m = bc.dyadic_poses(12)
    pred = (1.5 * m).astype(F)
    assert np.array_equal(pred.astype(F64), 1.5 * m)
    r32, r64, b = _both(pred, gt)
    y = m - m[:, :1]
    len_gt = np.stack([np.linalg.norm(y[:, j] - y[:, bc.PARENT[j]], axis=1) for j in range(1, 17)], 1)
    want = {'len_gt': len_gt, 'len_pred': 1.5 * len_gt, 'ang': 0 * len_gt, 'ang_pa': 0 * len_gt, 'e_dir': np.zeros((12, 17)),
            'e_len': 0.5 * np.linalg.norm(y, axis=2)}
    for name, w in want.items():
        d64, d32 = np.abs(bc.block(r64, name) - w).max(), np.abs(bc.block(r32, name) - w).max()
        print(f'{name}: float64 {d64:.3e}, float32 {d32:.3e}, bound {b[name]:.3e}')
        assert d64 <= (1e-7 if name == 'ang_pa' else 1e-12) and d32 <= b[name], name
    assert not bc.block(r32, 'ang').any() and not bc.block(r64, 'ang').any()           # parallel dyadic bones: the cross product is 0 exactly
    dlen32 = np.abs(bc.block(r32, 'len_pred') - bc.block(r32, 'len_gt'))
    assert np.abs(dlen32 - 0.5 * len_gt).max() <= b['len_pred'] + b['len_gt']


def test_a_rotated_skeleton_has_the_lengths_and_a_known_angle():
    """a 3-4-5 rotation about z through the pelvis of coordinates that are multiples of 5 / 1024: exact in float32"""
    gt, m = bc.dyadic_poses(12, seed=2, multiple=5)
    m[:, 1, 2] = m[:, 0, 2]                                                          # bone 1 (pelvis -> R_Hip) perpendicular to the axis
    gt = (m * 1000.0).astype(F)
    assert np.array_equal((gt / F(1000)).astype(F64), m)
    c = m - m[:, :1]
    rot = np.stack([(3 * c[..., 0] - 4 * c[..., 1]) / 5, (4 * c[..., 0] + 3 * c[..., 1]) / 5, c[..., 2]], -1) + m[:, :1]
    pred = rot.astype(F)
    assert np.array_equal(pred.astype(F64), rot)
    theta = math.atan2(4.0, 3.0)
    r32, r64, b = _both(pred, gt)
    for r, tol in ((r64, {k: 1e-12 for k in b}), (r32, b)):
        assert np.abs(bc.block(r, 'len_pred') - bc.block(r64, 'len_gt')).max() <= tol['len_pred']
        assert bc.block(r, 'e_len').max() <= tol['e_len']
        assert bc.block(r, 'ang_pa').max() <= max(tol['ang_pa'], 1e-7)
        assert np.abs(bc.block(r, 'ang')[:, 0] - theta).max() <= tol['ang']
    print(f'ang of the perpendicular bone against atan2(4, 3): float32 {np.abs(bc.block(r32, "ang")[:, 0] - theta).max():.3e} (bound {b["ang"]:.3e}); '
          f'ang_pa float32 {bc.block(r32, "ang_pa").max():.3e} (bound {b["ang_pa"]:.3e})')
    assert bc.block(r64, 'e_dir')[:, 1:].min() > 1e-3                                # the directions are what is wrong


@pytest.mark.parametrize('dtype', [F, F64])
def test_moving_either_pelvis_changes_nothing(dtype):
    rng = np.random.RandomState(5)
    gt, m = bc.dyadic_poses(12)
    _, other = bc.dyadic_poses(12, seed=9)
    pred = other.astype(F)
    base = bc.bones(pred, gt, dtype)
    assert bc.block(base, 'ang').min() > 0 and bc.block(base, 'e_dir')[:, 1:].min() > 0
    walk_p = rng.randint(-2048, 2048, size=(12, 1, 3)) / 1024.0                      # dyadic, the same for every joint: exact
    walk_g = rng.randint(-2048, 2048, size=(12, 1, 3)) / 1024.0
    pred2, gt2 = (other + walk_p).astype(F), ((m + walk_g) * 1000.0).astype(F)
    assert np.array_equal(pred2.astype(F64), other + walk_p) and np.array_equal((gt2 / F(1000)).astype(F64), m + walk_g)
    for p, g in ((pred2, gt), (pred, gt2), (pred2, gt2)):
        assert np.array_equal(bc.bones(p, g, dtype), base)


# ---- 2. derive and rigidity ----
def test_derive_and_rigidity_on_a_hand_made_table():
    br = _mod('bones_report')
    assert (br.ROW, br.TRAILER, br.COUNT, br.BAD, br.SUM_LEN_PRED, br.SUM_LEN_GT, br.SUM_ABS_DLEN, br.SUM_ANG, br.SUM_ANG_PA, br.SUM_SQ_PRED, br.SUM_SQ_GT,
            br.SUM_Q_PRED, br.SUM_Q_GT, br.SUM_ERR_DIR, br.SUM_ERR_LEN, br.SUM_ASYM_PRED, br.SUM_ASYM_GT) == \
        (bc.ROW, bc.TRAILER, bc.COUNT, bc.BAD, bc.SUM_LEN_PRED, bc.SUM_LEN_GT, bc.SUM_ABS_DLEN, bc.SUM_ANG, bc.SUM_ANG_PA, bc.SUM_SQ_PRED, bc.SUM_SQ_GT,
         bc.SUM_Q_PRED, bc.SUM_Q_GT, bc.SUM_ERR_DIR, bc.SUM_ERR_LEN, bc.SUM_ASYM_PRED, bc.SUM_ASYM_GT)
    assert br.PARENT == bc.PARENT and br.PAIRS == bc.PAIRS and len(br.BONE_NAMES) == 16 and br.BONE_NAMES[10] == 'Neck-L_Shoulder'
    one = 1 << 24
    table = np.zeros(2 * bc.ROW + 2, dtype=np.int64)
    a = table[:bc.ROW]
    a[bc.COUNT], a[bc.BAD] = 4, 1
    a[bc.SUM_LEN_GT:bc.SUM_LEN_GT + 16] = 4 * one // 4                               # every true bone 250 mm
    a[bc.SUM_LEN_PRED:bc.SUM_LEN_PRED + 16] = 4 * one // 4 + np.arange(16) * 4 * one // 1000      # bone i: i mm longer (truncated)
    a[bc.SUM_ABS_DLEN:bc.SUM_ABS_DLEN + 16] = 4 * one // 100                         # 10 mm
    a[bc.SUM_ANG:bc.SUM_ANG + 16] = int(round(4 * one * math.pi / 6))                # 30 degrees
    a[bc.SUM_ANG_PA:bc.SUM_ANG_PA + 16] = int(round(4 * one * math.pi / 18))         # 10 degrees
    a[bc.SUM_ERR_DIR:bc.SUM_ERR_DIR + 17] = np.arange(17) * (4 * one // 1000)        # joint j: j mm
    a[bc.SUM_ERR_LEN + 1:bc.SUM_ERR_LEN + 17] = 4 * one // 50                        # 20 mm on 16 joints, 0 at the pelvis
    a[bc.SUM_ASYM_PRED:bc.SUM_ASYM_PRED + 6] = 4 * one // 200                        # 5 mm
    # bone 0: lengths q = 100, 100, 300, 300 (units of 2^-16 m): mean 200, standard deviation 100; bone 1: four times 7: rigid
    a[bc.SUM_Q_PRED], a[bc.SUM_SQ_PRED] = 800, 2 * 100 ** 2 + 2 * 300 ** 2
    a[bc.SUM_Q_PRED + 1], a[bc.SUM_SQ_PRED + 1] = 28, 4 * 49
    a[bc.SUM_Q_GT:bc.SUM_Q_GT + 16], a[bc.SUM_SQ_GT:bc.SUM_SQ_GT + 16] = 4 * 16384, 4 * 16384 ** 2      # the true skeleton: rigid
    table[2 * bc.ROW] = 5
    doc = br.derive(table, ['S9', 'S11'])
    e = doc['groups']['S9']
    assert (e['n'], e['n_bad'], doc['ignored']) == (4, 1, 5)
    np.testing.assert_allclose(e['len_gt_mm'], [250.0] * 16, atol=1e-3)
    np.testing.assert_allclose(e['bias_mm'], np.arange(16.0), atol=1e-3)
    np.testing.assert_allclose([e['mean_len_gt_mm'], e['mean_len_pred_mm'], e['mean_bias_mm'], e['mean_abs_dlen_mm']], [250.0, 257.5, 7.5, 10.0], atol=1e-3)
    np.testing.assert_allclose([e['mean_ang_deg'], e['mean_ang_pa_deg'], e['ang_deg'][3]], [30.0, 10.0, 30.0], atol=1e-5)
    np.testing.assert_allclose(e['err_true_lengths_per_joint_mm'], np.arange(17.0), atol=1e-3)
    np.testing.assert_allclose([e['mpjpe_true_lengths_mm'], e['mpjpe_true_directions_mm']], [8.0, 20.0 * 16 / 17], atol=1e-3)      # / 17, the pelvis included
    np.testing.assert_allclose(e['asym_pred_mm'] + e['asym_gt_mm'], [5.0] * 6 + [0.0] * 6, atol=1e-3)
    w = doc['groups']['S11']
    assert (w['n'], w['len_pred_mm'], w['mean_ang_deg'], w['mpjpe_true_lengths_mm'], w['asym_gt_mm']) == (0, None, None, None, None)
    assert doc['all']['n'] == 4 and doc['all']['mpjpe_true_lengths_mm'] == e['mpjpe_true_lengths_mm']
    rig = br.rigidity({'before': table, 'after': table}, ['S9', 'S11'], ['before', 'after'])
    s9 = rig['per_subject']['S9']
    assert s9['after_mm'][0] == 100 / 65536 * 1000 and s9['after_mm'][1] == 0.0 and s9['gt_mm'] == [0.0] * 16 and s9['n'] == {'before': 4, 'after': 4}
    assert rig['per_subject']['S11']['gt_mm'] == [None] * 16 and rig['mean_gt_mm'] == 0.0
    assert abs(rig['mean_after_mm'] - 100 / 65536 * 1000 / 16) < 1e-12
    assert br.std_mm(3, 6, 14) == math.sqrt(6) / 3 / 65536 * 1000 and br.std_mm(0, 0, 0) is None      # 1, 2, 3
    table[2 * bc.ROW + 1] = 1
    with pytest.raises(RuntimeError, match='1 poses carried a group id outside'):
        br.derive(table, ['S9', 'S11'])
    with pytest.raises(RuntimeError, match='1 poses carried a subject id outside'):
        br.rigidity({'a': table}, ['S9', 'S11'], ['a'])
    with pytest.raises(ValueError, match='int64 expected for 3 groups'):
        br.derive(table, ['a', 'b', 'c'])


def test_the_integer_accumulation_adds_each_pose_to_one_class_of_words():
    pred, gt, group, special = bc.table_case()
    vals = bc.bones(pred, gt, F)
    table = bc.as_int64(bc.accumulate(vals, group, 3))
    t = table[:-2].reshape(3, bc.ROW)
    assert table[-2:].tolist() == [2, 1] and not t[1].any()
    assert int(t[:, bc.BAD].sum()) == 3 and int(t[:, bc.COUNT].sum()) == 65 - 3 - 3
    for name in ('nan', 'zero_bone', 'constant_pred'):
        i = special[name]
        alone = bc.as_int64(bc.accumulate(vals[i:i + 1], group[i:i + 1], 3))
        assert int(alone.sum()) == 1 and int(alone[int(group[i]) * bc.ROW + bc.BAD]) == 1, name
    halves = bc.accumulate(vals[30:], group[30:], 3, bc.accumulate(vals[:30], group[:30], 3))
    assert halves == table.tolist()
    perm = np.random.RandomState(1).permutation(65)
    assert bc.accumulate(vals[perm], group[perm], 3) == table.tolist()


# ---- 3. the flag ----
def _with_args(flags, fn):
    a = _mod('args')
    saved = a._LazyArgs._ns
    a._LazyArgs._ns = a.get_args(flags)
    try:
        return fn()
    finally:
        a._LazyArgs._ns = saved


def test_the_flag_defaults_to_off_and_names_what_it_needs(tmp_path):
    a, br = _mod('args'), _mod('bones_report')
    ns = a.get_args([])
    assert ns.eval_bones is False and a.get_args(['--eval_bones']).eval_bones is True
    for k, v in a.REFERENCE_FLAGS.items():
        assert getattr(ns, k) == v, k
    assert 'eval_bones' not in br.flags_doc(ns) and set(br.flags_doc(ns)) == set(vars(ns)) - {'eval_bones'}
    assert br.flags_doc({'eval_bones': True, 'lr': 1}) == {'lr': 1}
    br.check_flags(ns)
    br.check_flags(a.get_args(['--eval_bones', '--eval_report', 'dir']))
    with pytest.raises(ValueError, match='--eval_bones needs --eval_report DIR'):
        br.check_flags(a.get_args(['--eval_bones']))
    with pytest.raises(ValueError, match='--eval_bones needs --eval_report DIR'):
        _with_args(['--eval_bones', '--synthetic'], lambda: _mod('test').test_pose_refiner_model(log=lambda s: None))
    with pytest.raises(ValueError, match='--eval_bones needs --eval_report DIR'):
        _with_args(['--eval_bones', '--eval_vertices', str(tmp_path), '--regressor_report', str(tmp_path / 'out')],
                   lambda: _mod('eval_report').evaluate_vertices(log=lambda s: None))
    assert not os.path.exists(tmp_path / 'out')
    assert _mod('eval_report').read_optional_paths(str(tmp_path), 2) is None
    (tmp_path / 'paths.txt').write_text('a\nb\n')
    assert _mod('eval_report').read_optional_paths(str(tmp_path), 2) == ['a', 'b']
    with pytest.raises(ValueError, match='2 lines for 3 meshes'):
        _mod('eval_report').read_optional_paths(str(tmp_path), 3)
    main = open(os.path.join(ROOT, 'main.py')).read()
    assert re.search(r"\.bones_report'\)\.check_flags\(args\._get\(\)\)", main)


# ---- 4. the C ABI ----
def test_symbols_declared_exported_and_their_argument_checks():
    import ctypes
    hdr = open(os.path.join(ROOT, 'include', 'jrr.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    lib_mod, engine = _mod('_lib'), _mod('engine')
    _mod('build').build(verbose=False)
    lib = lib_mod.load()
    for name in ('jrr_bone_error', 'jrr_bone_accumulate'):
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in lib_mod.SIGNATURES and hasattr(lib, name)
    assert re.search(r'\|[^|\n]*`jrr_bone_error / _accumulate`[^|\n]*\|', doc) and 'bones.hip' in _mod('build').SOURCES
    consts = {k: int(v) for k, v in re.findall(r'\b(JRR_BONE_[A-Z0-9_]+) = (\d+)\b', hdr)}
    assert consts == {'JRR_BONE_ACC_LAYOUT_VERSION': _mod('bones_report').LAYOUT_VERSION, 'JRR_BONE_BONES': 16, 'JRR_BONE_PAIRS': 6, 'JRR_BONE_VALS': bc.VALS,
                      'JRR_BONE_LEN_PRED': bc.LEN_PRED, 'JRR_BONE_LEN_GT': bc.LEN_GT, 'JRR_BONE_ANG': bc.ANG, 'JRR_BONE_ANG_PA': bc.ANG_PA,
                      'JRR_BONE_ERR_DIR': bc.ERR_DIR, 'JRR_BONE_ERR_LEN': bc.ERR_LEN, 'JRR_BONE_ACC_ROW': bc.ROW, 'JRR_BONE_ACC_COUNT': bc.COUNT,
                      'JRR_BONE_ACC_BAD': bc.BAD, 'JRR_BONE_ACC_SUM_LEN_PRED': bc.SUM_LEN_PRED, 'JRR_BONE_ACC_SUM_LEN_GT': bc.SUM_LEN_GT,
                      'JRR_BONE_ACC_SUM_ABS_DLEN': bc.SUM_ABS_DLEN, 'JRR_BONE_ACC_SUM_ANG': bc.SUM_ANG, 'JRR_BONE_ACC_SUM_ANG_PA': bc.SUM_ANG_PA,
                      'JRR_BONE_ACC_SUM_SQ_PRED': bc.SUM_SQ_PRED, 'JRR_BONE_ACC_SUM_SQ_GT': bc.SUM_SQ_GT, 'JRR_BONE_ACC_SUM_Q_PRED': bc.SUM_Q_PRED,
                      'JRR_BONE_ACC_SUM_Q_GT': bc.SUM_Q_GT, 'JRR_BONE_ACC_SUM_ERR_DIR': bc.SUM_ERR_DIR, 'JRR_BONE_ACC_SUM_ERR_LEN': bc.SUM_ERR_LEN,
                      'JRR_BONE_ACC_SUM_ASYM_PRED': bc.SUM_ASYM_PRED, 'JRR_BONE_ACC_SUM_ASYM_GT': bc.SUM_ASYM_GT, 'JRR_BONE_ACC_TRAILER': bc.TRAILER}
    assert (engine.BONE_VALS, engine.BONE_ACC_ROW, engine.BONE_ACC_TRAILER) == (bc.VALS, bc.ROW, bc.TRAILER)
    parents = re.search(r'parent = \{([^}]*)\}', hdr).group(1)
    assert tuple(int(x) for x in parents.split(',')) == bc.PARENT
    assert all(f'({l},{r})' in hdr for l, r in bc.PAIRS)
    # argument errors come back as a status, nothing is launched (the pointers are never read)
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    err = lambda **kw: lib.jrr_bone_error(*[dict(dict(pred=p, gt=p, n=0, vals=p, stream=None), **kw)[k] for k in ('pred', 'gt', 'n', 'vals', 'stream')])
    assert err() == 0                                                                # batch == 0: no launch
    for k in ('pred', 'gt'):
        assert err(**{k: None}) == -1 and b'jrr_bone_error: bad argument' in lib.jrr_last_error(), k
    assert err(vals=None) == -1 and b'jrr_bone_error: no output' in lib.jrr_last_error()
    assert err(n=-1) == -1 and b'batch' in lib.jrr_last_error()
    for k in ('pred', 'gt', 'vals'):
        assert err(**{k: odd}) == -1 and b'4-byte aligned' in lib.jrr_last_error(), k
    acc = lambda **kw: lib.jrr_bone_accumulate(*[dict(dict(vals=p, grp=p, n=0, ng=3, acc=p, stream=None), **kw)[k] for k in ('vals', 'grp', 'n', 'ng', 'acc', 'stream')])
    assert acc() == 0 and acc(grp=None) == 0 and acc(ng=1) == 0 and acc(ng=1024) == 0
    for k in ('vals', 'acc'):
        assert acc(**{k: None}) == -1 and b'jrr_bone_accumulate: bad argument' in lib.jrr_last_error(), k
    assert acc(n=-1) == -1 and b'batch' in lib.jrr_last_error()
    assert acc(ng=0) == -1 and b'n_groups 0' in lib.jrr_last_error() and acc(ng=1025) == -1 and b'n_groups 1025' in lib.jrr_last_error()
    for kw in ({'vals': odd}, {'grp': odd}, {'acc': ctypes.c_void_p(4100)}):
        assert acc(**kw) == -1 and b'aligned' in lib.jrr_last_error(), kw


# ---- 5. bones_report end to end on CPU tensors ----
def _patch(monkeypatch):
    monkeypatch.setattr(_mod('engine'), 'bone_error', bc.host_bone_error)
    monkeypatch.setattr(_mod('engine'), 'bone_accumulate', bc.host_bone_accumulate)


def test_report_end_to_end_on_cpu_tensors(tmp_path, monkeypatch):
    br, er = _mod('bones_report'), _mod('eval_report')
    _patch(monkeypatch)
    before, after, gt, paths = bc.report_case()
    names, gids = er.assign_groups(paths, 'action')
    subjects, sids = br.subjects_of(paths)
    assert names == ['Eating', 'Walking'] and subjects == ['S11', 'S9']
    gids = gids.copy()
    gids[3] = -1                                                                     # a sample the dataset marks invalid
    sids = np.where(gids >= 0, sids, -1).astype(np.int32)
    report = br.BoneReport(names, subjects, 'cpu')
    assert report.acc.numel() == 2 * (2 * bc.ROW + 2 + 2 * bc.ROW + 2)                # ONE tensor: two tables per prediction set
    bc.fill(report, before, after, gt, gids, sids, 0, 40)
    res = report.finish(reduce=False)
    fake_eval = {k: {'all': {'mpjpe_mm': 50.0 + i}, 'groups': {g: {'mpjpe_mm': 40.0 + i} for g in names}} for i, k in enumerate(('before', 'after'))}
    doc = br.write(str(tmp_path / 'out'), res, 'action', 'parameters', fake_eval)
    assert sorted(os.listdir(tmp_path / 'out')) == ['bones.json', 'bones.md']
    back = br.load(str(tmp_path / 'out'))
    assert back == json.loads(json.dumps(doc)) and back['layout_version'] == 1 and back['parent'] == list(bc.PARENT) and len(back['bones']) == 16
    # the numbers: the float64 restatement's means over the scored poses
    keep = gids >= 0
    for which, pred in (('before', before), ('after', after)):
        r64, r32 = bc.bones(pred, gt, F64), bc.bones(pred, gt, F)
        b = bc.block_bounds(r32, r64)
        a = back['sets'][which]['all']
        assert a['n'] == 39 and a['n_bad'] == 0 and back['sets'][which]['ignored'] == 1 and a['mpjpe_mm'] == fake_eval[which]['all']['mpjpe_mm']
        step = 2.0 ** -25                                                            # half a unit of the fixed-point sums
        for key, name, unit in (('len_pred_mm', 'len_pred', 1000.0), ('len_gt_mm', 'len_gt', 1000.0), ('ang_deg', 'ang', 180 / math.pi),
                                ('ang_pa_deg', 'ang_pa', 180 / math.pi)):
            np.testing.assert_allclose(a[key], bc.block(r64, name)[keep].mean(0) * unit, rtol=0, atol=unit * (b[name] + step))
        dl = np.abs(bc.block(r64, 'len_pred') - bc.block(r64, 'len_gt'))[keep]
        np.testing.assert_allclose(a['abs_dlen_mm'], dl.mean(0) * 1000, rtol=0, atol=1000 * (b['len_pred'] + b['len_gt'] + step))
        np.testing.assert_allclose(a['bias_mm'], (bc.block(r64, 'len_pred') - bc.block(r64, 'len_gt'))[keep].mean(0) * 1000, rtol=0,
                                   atol=1000 * (b['len_pred'] + b['len_gt'] + 2 * step))
        assert abs(a['mpjpe_true_lengths_mm'] - bc.block(r64, 'e_dir')[keep].mean() * 1000) <= 1000 * (b['e_dir'] + step)
        assert abs(a['mpjpe_true_directions_mm'] - bc.block(r64, 'e_len')[keep].mean() * 1000) <= 1000 * (b['e_len'] + step)
        for k, (left, right) in enumerate(bc.PAIRS):
            want = np.abs(bc.block(r64, 'len_pred')[keep, left - 1] - bc.block(r64, 'len_pred')[keep, right - 1]).mean() * 1000
            assert abs(a['asym_pred_mm'][k] - want) <= 1000 * (2 * b['len_pred'] + step)
        g = back['sets'][which]['groups']
        assert g['Eating']['n'] + g['Walking']['n'] == 39 and g['Eating']['mpjpe_mm'] == fake_eval[which]['groups']['Eating']['mpjpe_mm']
    # rigidity: the planted ground truth is rigid, exactly; the predictions are not; 1.1 x a rigid skeleton + noise is less rigid than + less noise
    rig = back['rigidity']
    assert rig['mean_gt_mm'] == 0.0 and all(e['gt_mm'] == [0.0] * 16 for e in rig['per_subject'].values())
    assert rig['mean_before_mm'] > rig['mean_after_mm'] > 0 and rig['per_subject']['S9']['n'] == {'before': 19, 'after': 19}
    lp = bc.block(bc.bones(after, gt, F64), 'len_pred')
    sel = keep & (np.arange(40) >= 20)                                               # S11: the second half
    np.testing.assert_allclose(rig['per_subject']['S11']['after_mm'], lp[sel].std(0) * 1000, rtol=0, atol=1000 * 2.0 ** -15)
    md = open(tmp_path / 'out' / 'bones.md', encoding='utf-8').read()
    a0, a1 = back['sets']['before']['all'], back['sets']['after']['all']
    assert f"| all | 39 | 0 | 50.00 → 51.00 | {a0['mpjpe_true_lengths_mm']:.2f} → {a1['mpjpe_true_lengths_mm']:.2f} |" in md
    assert '| Neck-L_Shoulder |' in md and '| thigh |' in md and '| S11 | 20 |' in md and md.rstrip('\n').endswith(br.summary_line(back))
    assert br.summary_line(back).startswith('bones: before |Δ length| ') and 'rigidity' in br.summary_line(back)
    # without frame paths: no subject table, and the report says so
    plain = br.BoneReport(names, None, 'cpu')
    assert plain.acc.numel() == 2 * (2 * bc.ROW + 2)
    bc.fill(plain, before, after, gt, gids, None, 0, 40)
    res0 = plain.finish(reduce=False)
    assert res0['rigidity'] is None and res0['sets']['after']['all']['raw'] == res['sets']['after']['all']['raw']
    doc0 = br.write(str(tmp_path / 'plain'), res0, 'action', 'vertices')
    assert 'no frame paths' in open(tmp_path / 'plain' / 'bones.md', encoding='utf-8').read() and doc0['rigidity_note'].startswith('no frame paths')
    with pytest.raises(ValueError, match='subject ids go with'):
        plain.add('before', T(before[:2]), T(gt[:2]), T(gids[:2].copy()), T(sids[:2].copy()))
    # a group id outside the table is reported, not averaged away
    wrong = br.BoneReport(names, None, 'cpu')
    wrong.add('before', T(before[:2]), T(gt[:2]), T(np.array([0, 2], dtype=np.int32)))
    with pytest.raises(RuntimeError, match='1 poses carried a group id outside'):
        wrong.finish(reduce=False)
    back['layout_version'] = 2
    json.dump(back, open(tmp_path / 'out' / 'bones.json', 'w'))
    with pytest.raises(ValueError, match='layout version 2'):
        br.load(str(tmp_path / 'out'))


_RANK_WORKER = r'''
import importlib, os, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import torch.distributed as dist
import bone_cases as bc
br = importlib.import_module("joint-regressor-refinement_amd.bones_report")
er = importlib.import_module("joint-regressor-refinement_amd.eval_report")
eng = importlib.import_module("joint-regressor-refinement_amd.engine")
eng.bone_error, eng.bone_accumulate = bc.host_bone_error, bc.host_bone_accumulate
dist.init_process_group("gloo")
rank = dist.get_rank()
before, after, gt, paths = bc.report_case()
names, gids = er.assign_groups(paths, "action")
subjects, sids = br.subjects_of(paths)
report = br.BoneReport(names, subjects, "cpu")
bc.fill(report, before, after, gt, gids, sids, *((0, 23) if rank == 0 else (23, 40)))      # disjoint shards of the poses
br.write(os.path.join(sys.argv[2], "rank%d" % rank), report.finish(), "action", "vertices")
dist.barrier()
dist.destroy_process_group()
'''


def test_two_gloo_ranks_write_the_bytes_of_one_process(tmp_path, monkeypatch):
    br, er = _mod('bones_report'), _mod('eval_report')
    _patch(monkeypatch)
    before, after, gt, paths = bc.report_case()
    names, gids = er.assign_groups(paths, 'action')
    subjects, sids = br.subjects_of(paths)
    report = br.BoneReport(names, subjects, 'cpu')
    bc.fill(report, before, after, gt, gids, sids, 0, 40)
    br.write(str(tmp_path / 'one'), report.finish(), 'action', 'vertices')
    script = tmp_path / 'bones_rank_worker.py'
    script.write_text(_RANK_WORKER)
    out = str(tmp_path / 'two')
    os.makedirs(out)
    port = '29591'
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=port, OMP_NUM_THREADS='2')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
           '--master-port', port, str(script), ROOT, out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ['rank0']                                      # rank 0 alone wrote
    for name in ('bones.json', 'bones.md'):
        assert open(os.path.join(out, 'rank0', name), 'rb').read() == open(tmp_path / 'one' / name, 'rb').read(), name
