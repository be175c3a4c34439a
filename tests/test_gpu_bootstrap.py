"""The paired bootstrap on the GPU (pytest -m gpu): jrr_bootstrap_sums and jrr_paired_units against the numpy restatement
(tests/bootstrap_cases.py), the existing evaluation table, and `--eval_ci` through the mesh evaluation.

Bounds: none.  Everything behind the fp32 per-joint errors is an integer, so every comparison here is exact equality.

Shapes: ten segments of 0, 1, 3, 4, 5, 63, 64, 65, 257 and 1000 units in one call (a lane's Philox block is four draws, a wave's pass 256),
37 replicates from replicate 11, unit words above 2^40, a seed with a non-zero high word; 130 poses (three workgroups of 64, the last with
two) into 9 units and 3 groups."""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest
import torch

import bootstrap_cases as bc
import eval_report_cases as erc
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
F, F64 = np.float32, np.float64
PATTERN = 0x5a5a5a5a5a5a5a5a


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


# ---- 1. jrr_bootstrap_sums ----
@pytest.fixture(scope='module')
def kernel():
    """the case on the device and what the restatement says about it (computed once, never changed)"""
    units, segments = bc.kernel_case()
    return {'units': units, 'segments': segments, 'dev': T(units).to(DEV),
            'want': bc.bootstrap_sums(units, segments, bc.KERNEL_SEED, bc.KERNEL_REP_BEGIN, bc.KERNEL_REPS)}


def test_sums_equal_the_restatement_and_every_word_is_stored(kernel):
    out = torch.full((len(bc.SEGMENT_COUNTS), bc.KERNEL_REPS, 5), PATTERN, dtype=torch.int64, device=DEV)
    got = _mod('engine').bootstrap_sums(kernel['dev'], kernel['segments'], bc.KERNEL_SEED, bc.KERNEL_REP_BEGIN, bc.KERNEL_REPS, out=out)
    got = got.cpu().numpy()
    assert not (got == PATTERN).any() and not got[0].any()                   # the segment of no unit: zero rows, stored
    for s, count in enumerate(bc.SEGMENT_COUNTS):
        assert np.array_equal(got[s], kernel['want'][s]), f'segment {s} of {count} units'
    assert int(got[-1, :, :4].min()) > 1000 << 40                            # 1000 words above 2^40: beyond any 32-bit sum


def test_the_split_of_the_replicates_and_rep_begin_leave_every_bit_alone(kernel):
    eng = _mod('engine')
    b, n = bc.KERNEL_REP_BEGIN, bc.KERNEL_REPS
    halves = torch.cat([eng.bootstrap_sums(kernel['dev'], kernel['segments'], bc.KERNEL_SEED, b, 18),
                        eng.bootstrap_sums(kernel['dev'], kernel['segments'], bc.KERNEL_SEED, b + 18, n - 18)], dim=1).cpu().numpy()
    assert np.array_equal(halves, kernel['want'])
    from_zero = eng.bootstrap_sums(kernel['dev'], kernel['segments'], bc.KERNEL_SEED, 0, b + n).cpu().numpy()
    assert np.array_equal(from_zero[:, b:], kernel['want'])
    # a segment's rows depend on its own (s, begin, count): the same segment alone, in place 0, draws with s = 0 -- other bits
    other = eng.bootstrap_sums(kernel['dev'], kernel['segments'][5:6], bc.KERNEL_SEED, b, n).cpu().numpy()
    assert np.array_equal(other, bc.bootstrap_sums(kernel['units'], kernel['segments'][5:6], bc.KERNEL_SEED, b, n))
    assert not np.array_equal(other[0], kernel['want'][5])
    low = eng.bootstrap_sums(kernel['dev'], kernel['segments'], bc.KERNEL_SEED & 0xffffffff, b, n).cpu().numpy()
    assert not np.array_equal(low[1:], kernel['want'][1:])                   # the high word of the seed is part of the key


def test_bad_segments_are_refused_with_their_code_and_without_a_launch(kernel):
    lib, eng = _mod('_lib').load(), _mod('engine')
    P = ctypes.c_void_p
    out = torch.full((2, 3, 5), PATTERN, dtype=torch.int64, device=DEV)
    seg_dev = torch.zeros((2, 2), dtype=torch.int32, device=DEV)
    n_units = kernel['units'].shape[0]
    for rows, text in (([[0, 5], [3, -2]], b'negative count -2'), ([[0, 5], [n_units - 3, 4]], b'lies outside the table'), ([[-1, 3], [0, 1]], b'lies outside')):
        seg = np.ascontiguousarray(np.array(rows, dtype=np.int32))
        rc = lib.jrr_bootstrap_sums(P(kernel['dev'].data_ptr()), n_units, P(seg.ctypes.data), P(seg_dev.data_ptr()), 2, 5, 0, 3, P(out.data_ptr()), None)
        assert rc == -5 and text in lib.jrr_last_error(), (rows, lib.jrr_last_error())
    torch.cuda.synchronize()
    assert bool((out == PATTERN).all()) and not bool(seg_dev.any())          # nothing ran, nothing was uploaded
    with pytest.raises(OverflowError, match='2\\^62'):                       # the overflow rule, in Python integers, before the launch
        eng.bootstrap_sums(torch.full((4, 5), 1 << 52, dtype=torch.int64, device=DEV), [[0, 4], [0, 1 << 10]], 1, 0, 2)


# ---- 2. jrr_paired_units ----
@pytest.fixture(scope='module')
def poses():
    case = bc.pose_case()
    return {'np': case, 'dev': [T(a).to(DEV) for a in case], 'want': bc.paired_units(*case, bc.POSE_GROUPS, bc.POSE_UNITS)}


def _paired(dev, lo, hi, units=None, wins=None):
    units = torch.zeros((bc.POSE_UNITS, 5), dtype=torch.int64, device=DEV) if units is None else units
    wins = torch.zeros(bc.POSE_GROUPS * 8 + 3, dtype=torch.int64, device=DEV) if wins is None else wins
    _mod('engine').paired_units(*[t[lo:hi].contiguous() for t in dev], bc.POSE_GROUPS, units, wins)
    return units, wins


def test_units_and_wins_equal_the_restatement(poses):
    units, wins = _paired(poses['dev'], 0, bc.POSE_B)
    units, wins = units.cpu().numpy(), wins.cpu().numpy()
    want_units, want_wins = poses['want']
    assert np.array_equal(units, want_units) and np.array_equal(wins, want_wins)
    assert wins[-3:].tolist() == [1, 1, 1] and int(wins[:24].reshape(3, 8)[:, 1].sum()) == 1          # ignored, bad group, bad unit; the NaN pose
    assert int(units[4, 4]) == 70 - 1 and int(units[:, 4].sum()) == bc.POSE_B - 4                     # the unit across two workgroups (pose 77 left it)
    rows = wins[:24].reshape(3, 8)
    assert int(rows[:, 4].sum()) == 3 and int(rows[:, 7].sum()) == 3 and np.array_equal(rows[:, 2:5].sum(1), rows[:, 0]) and np.array_equal(rows[:, 5:8].sum(1), rows[:, 0])


def test_two_calls_over_a_split_batch_equal_one(poses):
    units, wins = _paired(poses['dev'], 0, 50)
    units, wins = _paired(poses['dev'], 50, bc.POSE_B, units, wins)
    assert np.array_equal(units.cpu().numpy(), poses['want'][0]) and np.array_equal(wins.cpu().numpy(), poses['want'][1])


# ---- 3. the units against the table of the existing report ----
def test_unit_columns_sum_to_the_sum_words_of_eval_accumulate():
    eng = _mod('engine')
    B, G = 200, 3
    pred, tgt = erc.pose_cases(B, seed=3)
    pred2 = (pred + np.random.RandomState(4).randn(*pred.shape).astype(F) * F(0.01)).astype(F)
    unit = (np.arange(B) // 4).astype(np.int32)                              # 50 units of 4 poses, unit u in group u % 3
    group = (unit % G).astype(np.int32)
    d_group, d_unit, gt = T(group).to(DEV), T(unit).to(DEV), T(tgt).to(DEV)
    errs, accs = [], []
    for p in (pred, pred2):
        e, e_pa = eng.evaluate_joints(T(p).to(DEV), gt)
        acc = torch.zeros(G * erc.ROW + erc.TRAILER, dtype=torch.int64, device=DEV)
        eng.eval_accumulate(e, e_pa, d_group, G, acc)
        errs += [e, e_pa]
        accs.append(acc.cpu().numpy()[:G * erc.ROW].reshape(G, erc.ROW))
    units = torch.zeros((50, 5), dtype=torch.int64, device=DEV)
    wins = torch.zeros(G * 8 + 3, dtype=torch.int64, device=DEV)
    eng.paired_units(*errs, d_group, d_unit, G, units, wins)
    units, wins = units.cpu().numpy(), wins.cpu().numpy()
    assert not accs[0][:, erc.BAD].any() and not accs[1][:, erc.BAD].any() and not wins[-3:].any()     # the inputs hold no bad pose
    for g in range(G):
        col = units[np.arange(50) % G == g].sum(0)
        assert int(col[0]) == int(accs[0][g, erc.SUM:erc.SUM + 17].sum()) and int(col[1]) == int(accs[0][g, erc.SUM_PA:erc.SUM_PA + 17].sum())
        assert int(col[2]) == int(accs[1][g, erc.SUM:erc.SUM + 17].sum()) and int(col[3]) == int(accs[1][g, erc.SUM_PA:erc.SUM_PA + 17].sum())
        assert int(col[4]) == int(accs[0][g, erc.COUNT]) == int(wins[g * 8])


# ---- 4. --eval_ci through the mesh evaluation ----
def _with_args(flags, fn):
    argsmod = _mod('args')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(flags + ['--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent', '--synthetic', '--device', DEV])
    try:
        torch.manual_seed(0)
        return fn()
    finally:
        argsmod._LazyArgs._ns = saved


def test_eval_ci_through_eval_vertices_equals_the_restatement_and_leaves_eval_json_alone(tmp_path, smpl_model_np, monkeypatch):
    """40 meshes: two actions of two cameras each and a stray without imageSequence -- 5 sequences, 3 groups.  ci.json holds the
    restatement's document on the same joints; eval.json / eval.md keep their bytes; `frame` units give 40 units."""
    n, reps, seed, level = 40, 200, 3, 0.9
    er, cr, eng, utils = _mod('eval_report'), _mod('ci_report'), _mod('engine'), _mod('utils')
    action = np.where(np.arange(n) < 20, 'Walking 1', 'Eating 2')
    paths = [f'/data/h36m/S9/{a}/imageSequence/{i % 2 + 1}/img_{5 * (i // 2 + 1):06d}.jpg' for i, a in enumerate(action)]
    paths[n - 1] = '/data/elsewhere/000001.jpg'
    J = _mod('smpl_model').default_h36m_regressor()
    J2 = (J * (1 + 0.5 * np.random.RandomState(5).rand(*J.shape))).astype(F)
    ck = str(tmp_path / 'retrained_J_Regressor.pt')
    _mod('checkpoint').save_j_regressor(T(J2), ck)
    rng = np.random.RandomState(11)
    t = (np.arange(n) // 2)[:, None, None]
    verts = (smpl_model_np['v_template'][None] + 0.02 * np.sin(0.4 * t + rng.uniform(0, 6, size=(1, 6890, 3))) + rng.normal(0, 0.002, size=(n, 6890, 3))).astype(F)
    gt = (np.einsum('jv,nvc->njc', J.astype(F64), verts.astype(F64)) * 1000 + rng.normal(0, 3, size=(n, 17, 3))).astype(F)
    vdir = str(tmp_path / 'meshes')
    os.makedirs(vdir)
    np.save(os.path.join(vdir, 'vertices.npy'), verts)
    np.save(os.path.join(vdir, 'gt_j3d.npy'), gt)
    with open(os.path.join(vdir, 'paths.txt'), 'w') as f:
        f.write('\n'.join(paths) + '\n')
    flags = ['--batch_size', '16', '--eval_j_regressor', ck, '--eval_vertices', vdir, '--seed', str(seed), '--eval_report', 'rep']
    ci = ['--eval_ci', '--eval_ci_reps', str(reps), '--eval_ci_level', str(level)]
    lines = {}
    for key, extra in (('plain', []), ('ci', ci), ('frame', ci + ['--eval_ci_unit', 'frame'])):
        os.makedirs(tmp_path / key)
        monkeypatch.chdir(tmp_path / key)                                    # the flag `--eval_report rep` is recorded: the same words in every run
        lines[key] = []
        _with_args(flags + extra, lambda: er.evaluate_vertices(log=lines[key].append))
    out = {key: str(tmp_path / key / 'rep') for key in lines}
    assert sorted(os.listdir(out['plain'])) == ['eval.json', 'eval.md'] and sorted(os.listdir(out['ci'])) == ['ci.json', 'ci.md', 'eval.json', 'eval.md']
    for name in ('eval.json', 'eval.md'):
        assert open(os.path.join(out['plain'], name), 'rb').read() == open(os.path.join(out['ci'], name), 'rb').read(), name
    assert 'eval_ci' not in json.load(open(os.path.join(out['ci'], 'eval.json')))['flags']
    assert lines['ci'][:2] == lines['plain'][:2] and lines['ci'][2].startswith('paired bootstrap, after - before in mm with the 90 % interval, 200 resamples of 5 sequences: MPJPE ')
    assert lines['ci'][3:] == lines['plain'][2:] and len(lines['plain']) == 3
    # the restatement's document on the same joints
    Js = torch.stack([T(J), T(J2)]).float().to(DEV)
    joints = eng.JointRegressorTable(Js, utils.find_j_reg_mask(Js[0])).regress(T(verts).to(DEV))
    gtc = utils.move_pelvis(T(gt).to(DEV))
    errs = [a.cpu().numpy() for k in (0, 1) for a in eng.evaluate_joints(joints[k].contiguous(), gtc)]
    names, group = er.assign_groups(paths, 'action')
    assert names == ['Eating', 'Walking', 'all']
    keys = sorted({p.rsplit('/', 1)[0] for p in paths[:-1]})
    unit = np.array([keys.index(p.rsplit('/', 1)[0]) for p in paths[:-1]] + [len(keys)], dtype=np.int32)
    group_of_unit = [int(group[np.nonzero(unit == u)[0][0]]) for u in range(5)]
    doc = cr.load(out['ci'])
    want = bc.document(*errs, group, unit, group_of_unit, names, 5, reps, seed, level, 'sequence')
    assert doc['data'] == json.loads(json.dumps(want)) and doc['source'] == 'vertices' and doc['groups'] == names
    r = doc['data']['all']
    assert r['n_units'] == 5 and r['n_poses'] == n and doc['data']['groups']['all']['n_units'] == 1 and r['mpjpe']['difference']['se_mm'] > 0
    print('sequence units: ' + lines['ci'][2])
    frame = cr.load(out['frame'])
    want = bc.document(*errs, group, np.arange(n, dtype=np.int32), [int(g) for g in group], names, n, reps, seed, level, 'frame')
    assert frame['data'] == json.loads(json.dumps(want)) and frame['data']['all']['n_units'] == n
    assert frame['data']['all']['raw_sums'] == r['raw_sums']                 # the same poses: the point estimate does not depend on the unit
    print('frame units:    ' + lines['frame'][2])
