"""The evaluation protocols without a GPU (`--eval_protocol`, `--eval_gt_joints`): the host restatement (tests/protocol_cases.py)
against the reference's stored values (g10, g11, g13), the presets, the divisors of `derive`, every refusal with its message, the
`--eval_vertices` directory without gt_j3d.npy, and what the flags add to the recorded flags at their defaults: nothing."""
import importlib
import os
import types

import numpy as np
import pytest
import torch

import eval_report_cases as ec
import protocol_cases as pc
from conftest import PKG_NAME, load_golden

F = np.float32


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _ns(**kw):
    base = dict(eval_protocol='h36m17', eval_gt_joints='file', eval_vertices=None, eval_report=None, eval_accel=False, eval_bones=False,
                regressor_report=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


# ---- 1. the restatement against the reference's values ----
def test_float32_restatement_reproduces_g13_bit_for_bit():
    g11, g13 = load_golden('g11_eval_degenerate.npz'), load_golden('g13_eval_protocol.npz')
    assert len(g13) == 2 * len(pc.G13_MASKS) * len(pc.ROOTS)
    for mask_name in pc.G13_MASKS:
        for root_name, root in pc.ROOTS.items():
            e, pa = pc.evaluate_protocol(g11['pred'], g11['target_mm'], pc.MASKS[mask_name], root, pc.TARGET_MM, torch.float32)
            assert e.dtype == F and np.array_equal(e, g13[pc.g13_key(mask_name, root_name, 'err_j')]), (mask_name, root_name)
            assert np.array_equal(pa, g13[pc.g13_key(mask_name, root_name, 'err_pa_j')]), (mask_name, root_name)
            out = [i for i in range(17) if i not in pc.joints_of(pc.MASKS[mask_name])]
            assert not e[:, out].any() and not pa[:, out].any() and (e[:, pc.joints_of(pc.MASKS[mask_name])] > 0).all()
            # the fixture's own condition: each family within its cap of the float64 restatement
            e64, pa64 = pc.evaluate_protocol(g11['pred'], g11['target_mm'], pc.MASKS[mask_name], root, pc.TARGET_MM, torch.float64)
            for k, name in enumerate(ec.G11_FAMILIES):
                sl = slice(k * ec.G11_POSES, (k + 1) * ec.G11_POSES)
                assert pc.distance(pa[sl], pa64[sl]) <= ec.FAMILIES[name][1] and pc.distance(e[sl], e64[sl]) <= ec.FAMILIES[name][1], name


def test_all17_joint0_millimetres_reproduces_g10_and_g11():
    for name in ('g10_eval_joints.npz', 'g11_eval_degenerate.npz'):
        g = load_golden(name)
        e, pa = pc.evaluate_protocol(g['pred'], g['target_mm'], pc.MASKS['all17'], pc.ROOT_JOINT0, pc.TARGET_MM, torch.float32)
        assert np.array_equal(e, g['err_j']) and np.array_equal(pa, g['err_pa_j']), name


def test_one_joint_gives_nan_aligned_and_finite_plain_distances_in_both_dtypes():
    pred, tgt, _, _ = ec.mixed_cases(28)
    for dtype in (torch.float32, torch.float64):
        e, pa = pc.evaluate_protocol(pred, tgt, pc.MASKS['one1'], pc.ROOT_HIPS, pc.TARGET_MM, dtype)
        assert np.isnan(pa[:, 10]).all() and np.isfinite(e).all() and not pa[:, :10].any() and not pa[:, 11:].any()


def test_metre_targets_and_the_masked_accumulate():
    pred, tgt, _, _ = ec.mixed_cases(28)
    e, pa = pc.evaluate_protocol(pred, tgt, pc.MASKS['lsp14'], pc.ROOT_HIPS, pc.TARGET_MM, torch.float64)
    em, pam = pc.evaluate_protocol(pred, tgt.astype(np.float64) / 1000, pc.MASKS['lsp14'], pc.ROOT_HIPS, pc.TARGET_M, torch.float64)
    assert np.array_equal(e, em) and np.array_equal(pa, pam, equal_nan=True)
    # at the full mask the masked accumulate is the existing one; under a mask the excluded words stay 0 and COUNT / BAD ignore them
    e0, e1, group = ec.accumulate_case()
    assert np.array_equal(pc.accumulate(e0, e1, group, 3, pc.MASKS['all17']), ec.accumulate(e0, e1, group, 3))
    mask = pc.MASKS['lsp14']
    t = pc.accumulate(e0, e1, group, 3, mask)
    rows = t[:3 * ec.ROW].reshape(3, ec.ROW)
    for j in (0, 7, 9):
        assert not rows[:, ec.SUM + j].any() and not rows[:, ec.SUM_PA + j].any()
    full = ec.accumulate(e0, e1, group, 3)[:3 * ec.ROW].reshape(3, ec.ROW)
    assert int(rows[:, ec.BAD].sum()) == int(full[:, ec.BAD].sum()) - 1          # accumulate_case's inf sits in joint 0: excluded, its pose counts
    assert np.array_equal(rows[:, ec.HIST:ec.HIST + ec.BINS].sum(1), 14 * rows[:, ec.COUNT])


# ---- 2. the presets ----
def test_preset_masks_and_names():
    ep, er = _mod('eval_protocol'), _mod('eval_report')
    assert tuple(ep.PRESETS) == ('h36m17', 'lsp14', 'lsp14_hips') and ep.DEFAULT == 'h36m17'
    h, l, v = (ep.PRESETS[k] for k in ep.PRESETS)
    assert (h.joint_mask, h.root, h.joints) == (0x1FFFF, ep.ROOT_JOINT0, tuple(range(17))) and h.is_default and h.n_joints == 17
    assert (l.joint_mask, l.root) == (0x1FD7E, ep.ROOT_JOINT0) and (v.joint_mask, v.root) == (0x1FD7E, ep.ROOT_HIPS)
    assert not l.is_default and not v.is_default and l.n_joints == v.n_joints == 14 and l.joints == v.joints
    # 0x1FD7E is exactly the 17 joints minus Pelvis, Torso and Nose
    assert [er.JOINT_NAMES[i] for i in range(17) if not 0x1FD7E >> i & 1] == ['Pelvis', 'Torso', 'Nose']
    assert 0x1FD7E == pc.MASKS['lsp14'] == ep.MASK_LSP14 and ep.MASK_ALL == pc.MASKS['all17'] and 0x1FD7E >> 17 == 0
    assert (er.JOINT_NAMES[1], er.JOINT_NAMES[4]) == ('R_Hip', 'L_Hip')          # the hips of ROOT_HIPS
    assert ep.Protocol('x', 0b110, 0, (1, 2)) == ep.make('x', 0b110, 0)
    for bad in (0, 1 << 17, -1):
        with pytest.raises(ValueError, match='joint mask'):
            ep.make('bad', bad, 0)
    with pytest.raises(ValueError, match='root'):
        ep.make('bad', 1, 2)
    with pytest.raises(ValueError, match='--eval_protocol'):
        ep.get('coco')
    args = _mod('args').get_args(['--eval_protocol', 'lsp14_hips', '--eval_gt_joints', 'regressed'])
    assert ep.of(args) is v and ep.gt_source(args) == 'regressed'
    d = _mod('args').get_args([])
    assert (d.eval_protocol, d.eval_gt_joints) == ('h36m17', 'file') and ep.is_default_run(d)


# ---- 3. derive under 14 joints ----
def test_derive_divides_by_the_protocols_joints_and_reports_none_for_the_others():
    ep, er = _mod('eval_protocol'), _mod('eval_report')
    proto = ep.PRESETS['lsp14']
    rs = np.random.RandomState(3)
    B, G = 40, 2
    e0, e1 = np.abs(rs.randn(B, 17) * 0.06).astype(F), np.abs(rs.randn(B, 17) * 0.03).astype(F)
    e0[:, [0, 7, 9]] = 0
    e1[:, [0, 7, 9]] = 0
    group = (np.arange(B) % G).astype(np.int32)
    table = pc.accumulate(e0, e1, group, G, proto.joint_mask)
    doc = er.derive(table, ['a', 'b'], proto)
    sel = list(proto.joints)
    for g, name in enumerate(['a', 'b']):
        r = doc['groups'][name]
        rows = group == g
        fixed = np.rint(e0[rows][:, sel].astype(np.float64) * (1 << 24))
        assert r['n'] == int(rows.sum()) and r['mpjpe_mm'] == float(fixed.sum() / (1 << 24) / (14 * r['n']) * 1000.0)
        assert [x is None for x in r['mpjpe_per_joint_mm']] == [i in (0, 7, 9) for i in range(17)]
        assert [x is None for x in r['pampjpe_per_joint_mm']] == [i in (0, 7, 9) for i in range(17)]
        assert abs(np.mean([x for x in r['mpjpe_per_joint_mm'] if x is not None]) - r['mpjpe_mm']) < 1e-9
        assert r['pck_mpjpe']['150'] == float((np.floor(e0[rows][:, sel] * F(1000)) < 150).sum() / (14 * r['n']))
    n, mp, pa = pc.means_mm(table, G, proto.joint_mask)
    assert [doc['groups'][k]['mpjpe_mm'] for k in ('a', 'b')] == mp.tolist() and [doc['groups'][k]['pampjpe_mm'] for k in ('a', 'b')] == pa.tolist()
    # without a protocol, and under h36m17, the same table is read as before: 17 in every divisor, no None
    full = pc.accumulate(e0, e1, group, G, ep.MASK_ALL)
    assert er.derive(full, ['a', 'b']) == er.derive(full, ['a', 'b'], ep.PRESETS['h36m17'])
    assert None not in er.derive(full, ['a', 'b'])['all']['mpjpe_per_joint_mm']
    # the bootstrap's means take the same divisor
    ci = _mod('ci_report')
    assert ci._mean_mm(14.0 * (1 << 24), 1.0, 14) == 1000.0 and ci._mean_mm(17.0 * (1 << 24), 1.0) == 1000.0
    # the markdown names the protocol and prints `-` for an excluded joint
    entry = ep.document(proto, 'file', er.JOINT_NAMES)
    assert entry == {'name': 'lsp14', 'joints': [er.JOINT_NAMES[i] for i in sel], 'joint_mask': 0x1FD7E, 'root': 'joint0', 'gt_joints': 'file'}
    md = er.markdown({'source': 'vertices', 'group_kind': 'none', 'groups': ['a', 'b'], 'joints': list(er.JOINT_NAMES), 'regressors': {'before': doc, 'after': doc},
                      'j_regressor_initial': {'path': 'i', 'sha256_16': 'x'}, 'j_regressor_retrained': {'path': 'r', 'sha256_16': 'y'}, 'protocol': entry})
    assert 'protocol lsp14' in md.splitlines()[0] and 'Protocol `lsp14`: 14 joints' in md and '| Pelvis | - → - → - | - → - → - |' in md
    assert 'on all 17 joints centred on joint 0' in md
    assert ep.document(None, 'file', er.JOINT_NAMES) is None and ep.document(ep.PRESETS['h36m17'], 'regressed', er.JOINT_NAMES)['gt_joints'] == 'regressed'


# ---- 4. the refusals ----
def test_every_refusal_names_its_flags(tmp_path):
    ep = _mod('eval_protocol')
    ep.check_flags(_ns())
    ep.check_flags(_ns(eval_protocol='lsp14_hips', eval_accel=True, eval_bones=True, regressor_report='r'))      # `file` ground truth: they run as today
    with pytest.raises(ValueError, match='--eval_gt_joints regressed needs --eval_vertices DIR'):
        ep.check_flags(_ns(eval_gt_joints='regressed'))
    empty = str(tmp_path / 'empty')
    os.makedirs(empty)
    with pytest.raises(FileNotFoundError, match=r'--eval_gt_joints regressed: .*gt_vertices\.npy is missing.*--eval_vertices'):
        ep.check_flags(_ns(eval_gt_joints='regressed', eval_vertices=empty))
    np.save(os.path.join(empty, 'gt_vertices.npy'), np.zeros((1, 6890, 3), dtype=F))
    ep.check_flags(_ns(eval_gt_joints='regressed', eval_vertices=empty))
    for flag, value in (('eval_accel', True), ('eval_bones', True), ('regressor_report', 'out')):
        with pytest.raises(ValueError, match=f'--eval_gt_joints regressed cannot go with --{flag}'):
            ep.check_flags(_ns(eval_gt_joints='regressed', eval_vertices=empty, **{flag: value}))
    with pytest.raises(ValueError, match='--eval_protocol'):
        ep.check_flags(_ns(eval_protocol='coco'))
    with pytest.raises(ValueError, match='--eval_gt_joints'):
        ep.check_flags(_ns(eval_gt_joints='guessed'))
    with pytest.raises(SystemExit):                                         # the command line offers the presets, no free-form joint list
        _mod('args').get_args(['--eval_protocol', '1,2,3'])


def test_open_vertices_dir_without_gt_j3d(tmp_path):
    er = _mod('eval_report')
    d = str(tmp_path / 'meshes')
    os.makedirs(d)
    np.save(os.path.join(d, 'vertices.npy'), np.zeros((3, 6890, 3), dtype=F))
    with pytest.raises(FileNotFoundError, match=r'--eval_vertices: .*gt_j3d\.npy is missing'):
        er.open_vertices_dir(d, 'none')
    with pytest.raises(FileNotFoundError, match=r'--eval_vertices: .*gt_j3d\.npy is missing'):
        er.open_vertices_dir(d, 'none', 'file')
    verts, gt, names, ids = er.open_vertices_dir(d, 'none', 'regressed')
    assert verts.shape == (3, 6890, 3) and gt is None and names == ['all'] and ids.tolist() == [0, 0, 0]
    np.save(os.path.join(d, 'gt_j3d.npy'), np.full((3, 17, 3), np.nan, dtype=F))      # present but NaN: refused in `file` mode, not read in `regressed`
    with pytest.raises(ValueError, match='NaN in the ground truth'):
        er.open_vertices_dir(d, 'none')
    assert er.open_vertices_dir(d, 'none', 'regressed')[1] is None


# ---- 5. the recorded flags ----
def test_flags_doc_adds_nothing_at_the_defaults():
    ep, args = _mod('eval_protocol'), _mod('args')
    d = vars(args.get_args([]))
    doc = ep.flags_doc(d)
    assert 'eval_protocol' not in doc and 'eval_gt_joints' not in doc and set(d) - set(doc) == {'eval_protocol', 'eval_gt_joints'}
    assert ep.flags_doc(vars(args.get_args(['--eval_protocol', 'h36m17', '--eval_gt_joints', 'file']))) == doc
    assert ep.flags_doc(args.get_args([])) == doc                            # a namespace as well
    for flags in (['--eval_protocol', 'lsp14'], ['--eval_gt_joints', 'regressed']):
        got = ep.flags_doc(vars(args.get_args(flags)))
        assert got['eval_protocol'] == (flags[1] if flags[0] == '--eval_protocol' else 'h36m17') and 'eval_gt_joints' in got
