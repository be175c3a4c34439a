"""The view fusion over the refined-pose table on the GPU (pytest -m gpu): jrr_view_relrot_accumulate and jrr_view_fuse against the float64
evaluation of the host restatement (tests/view_fuse_cases.py), the bit-level properties the header promises, the status bits, planted
truth, refined.fuse_views on a table the driver wrote from a dataset directory with a camera rig, and the `--fuse_refined` command.

Bounds: there is no reference implementation, so every comparison is held to `3 x (distance of the restatement's float32 evaluation
from its float64 evaluation on THIS test's inputs) + 1e-7` (view_fuse_cases.bound), the maximum over all entries; rotations are compared
as matrices, angles in radians.  The cases compared that way meet the branch conditions of view_fuse_cases (asserted in float64).

Shapes: a 96-row table, 70 listed rows in a non-monotone order with the unrefined rows in between, groups of 1, 2, 3, 4, 8, 4, 4, 8, ...
views (three workgroups of 32 positions, the last with 6; a group of 8 straddles each tile border), nine cameras of which one never meets
the reference camera.  Joints cycle through any angle / within 1e-3 of pi / the exact identity / views whose quaternions have opposite
signs.
"""
import importlib
import os
import pickle

import numpy as np
import pytest
import torch

import refined_cases as rc
import view_fuse_cases as vc
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
F = np.float32
NAMES = ('x6d', 'betas', 'body', 'orient', 'members', 'dropped')


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


class Case:
    """a case of view_fuse_cases on the device"""

    def __init__(self, c):
        self.c = c
        self.x6d, self.betas = vc.positions_of(c['table'], c['order'])
        self.dev = {k: T(np.ascontiguousarray(c[k])).to(DEV) for k in ('table', 'order', 'group', 'pair', 'ref_pair')}
        self.n_pairs = len(c['ref_pair'])

    def lists(self, **kw):
        return [T(np.ascontiguousarray(kw[k])).to(DEV) if k in kw else self.dev[k] for k in ('table', 'order', 'group', 'pair')]

    def fuse(self, max_deg, rel, begin=0, count=None, out=None, **kw):
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = _mod('engine').view_fuse(*self.lists(**kw), T(np.ascontiguousarray(rel, dtype=F)).to(DEV), vc.cos_half(max_deg), status,
                                       begin=begin, count=count, out=out)
        return {k: t.cpu().numpy() for k, t in zip(NAMES, out)}, int(status.item()), out

    def accumulate(self, begin=0, count=None, acc=None, ref_pair=None, **kw):
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        ref = self.dev['ref_pair'] if ref_pair is None else T(ref_pair).to(DEV)
        acc = torch.zeros((ref.shape[0], vc.ACC_ROW), dtype=torch.int64, device=DEV) if acc is None else acc
        _mod('engine').view_relrot_accumulate(*self.lists(**kw), ref, acc, status, begin=begin, count=count)
        return acc, int(status.item())


@pytest.fixture(scope='module')
def case():
    return Case(vc.table_case())


def _same_bits(a, b, rows_a=slice(None), rows_b=slice(None)):
    for k in NAMES:
        assert np.array_equal(_bits(a[k][rows_a]), _bits(b[k][rows_b])), k


def _check_against(got, want, d, what):
    g = vc.distances(got, want)
    for name, gv, dv in zip(('rotation', 'betas', 'body rad', 'orient rad'), g, d):
        print(f'{what}: {name} {gv:.3e} (yardstick {dv:.3e}, bound {vc.bound(dv):.3e})')
    for gv, dv in zip(g, d):
        assert gv <= vc.bound(dv)
    assert np.array_equal(got['members'], want['members']) and np.array_equal(got['dropped'], want['dropped'])


# ---- 1. both kernels against float64 ----
@pytest.mark.parametrize('max_deg', [0.0, 30.0])
def test_view_fuse_against_float64(case, max_deg):
    c = case.c
    before = case.dev['table'].clone()
    got, status, _ = case.fuse(max_deg, c['rel'])
    want, d, r32 = vc.yardstick(case.x6d, case.betas, c['group'], c['pair'], c['rel'], max_deg)
    assert status == 0
    _check_against(got, want, d, f'max_deg {max_deg:g}')
    assert torch.equal(case.dev['table'].view(torch.int32), before.view(torch.int32))       # the input table is unchanged byte for byte
    assert got['dropped'].sum() == (len(c['outliers']) if max_deg else 0)
    # every output is a rotation's first two columns, but where a row is copied; the identity joints stay the exact identity
    fused = r32['taken'] > 1
    R = vc.rot6d(got['x6d'])
    assert np.abs(R[..., :2] - got['x6d'].reshape(vc.M, 24, 3, 2))[fused].max() <= 1e-6
    assert np.array_equal(got['x6d'][:, 2::4], np.broadcast_to(F([1, 0, 0, 1, 0, 0]), (vc.M, 6, 6)))
    # every member of a group gets bit-identical body rotations and betas (a joint at which only one view is taken is that view's copy
    # in its own row, and its orthonormalised columns in the others')
    for first in np.nonzero(np.diff(c['group'], prepend=-1))[0]:
        n = vc.GROUP_SIZES[c['group'][first]]
        rows = slice(first, first + n)
        several = (r32['taken'][first, 1:] > 1) | (n == 1)
        assert (_bits(got['x6d'][rows, 1:])[:, several] == _bits(got['x6d'][first, 1:])[several]).all()
        assert (_bits(got['betas'][rows]) == _bits(got['betas'][first])).all()
    # a group of one is copied bit for bit, signed zeros included
    assert np.array_equal(_bits(got['x6d'][0]), _bits(case.x6d[0])) and np.array_equal(_bits(got['betas'][0]), _bits(case.betas[0]))
    assert np.signbit(got['betas'][0, 0]) and got['members'][0] == 1 and got['body'][0] <= 0.05
    # a position with an unknown pair keeps its orientation bits and gets NaN in delta_orient_deg
    lost = np.nonzero(c['pair'] == 8)[0]
    assert lost.size == 1 and np.isnan(got['orient'][lost]).all() and np.isnan(got['orient']).sum() == 1
    assert np.array_equal(_bits(got['x6d'][lost, 0]), _bits(case.x6d[lost, 0])) and not np.array_equal(got['x6d'][lost, 1], case.x6d[lost, 1])


def test_relrot_accumulate_against_float64(case):
    c = case.c
    before = case.dev['table'].clone()
    acc, status = case.accumulate()
    count, mean = vc.acc_mean(acc.cpu().numpy())
    count64, mean64 = vc.accumulate(case.x6d, c['group'], c['pair'], c['ref_pair'])
    count32, mean32 = vc.accumulate(case.x6d, c['group'], c['pair'], c['ref_pair'], F)
    d, g = vc.dist(mean32, mean64), vc.dist(mean, mean64)
    print(f'acc / (2^24 count): {g:.3e} (yardstick {d:.3e}, bound {vc.bound(d):.3e}); counts {count.tolist()}')
    assert status == 0 and np.array_equal(count, count64) and np.array_equal(count32, count64) and g <= vc.bound(d)
    assert count[0] == 0 and count[8] == 0 and (count[1:8] > 0).all() and not acc.cpu().numpy()[:, 11].any()
    assert torch.equal(case.dev['table'].view(torch.int32), before.view(torch.int32))
    rel, res = _mod('refined').relative_rotations(acc.cpu().numpy(), c['ref_pair'])
    mine = vc.solve(count64, mean64, c['ref_pair'])[0]
    assert not rel[8].any() and rel[0].tolist() == [1, 0, 0, 0] and np.abs(rel - mine).max() <= 1e-5


# ---- 2. a result depends on its group alone; the table on the multiset of positions ----
def test_split_shift_and_growth_give_equal_bits(case):
    c = case.c
    whole, _, _ = case.fuse(30.0, c['rel'])
    # two calls, split inside the group of 8 at positions 26 .. 33 (29 is no multiple of the tile)
    first, status, out = case.fuse(30.0, c['rel'], begin=0, count=29)
    assert np.isnan(first['body'][29:]).all() and np.isnan(first['x6d'][29:]).all() and not first['members'][29:].any()
    _same_bits(first, whole, slice(0, 29), slice(0, 29))
    both, status2, _ = case.fuse(30.0, c['rel'], begin=29, count=vc.M - 29, out=out)
    assert status == 0 and status2 == 0
    _same_bits(both, whole)
    # five single-view positions in front shift every tile; ten more behind let m grow
    spare = np.setdiff1d(np.arange(vc.N_ROWS), c['order'])[:5].astype(np.int32)
    table = c['table'].copy()
    table[spare] = table[c['order'][[3, 9, 20, 40, 60]]]
    singles = dict(group=np.arange(5, dtype=np.int32), pair=np.full(5, -1, np.int32))
    front = dict(table=table, order=np.concatenate([spare, c['order']]), group=np.concatenate([singles['group'], c['group'] + 5]),
                 pair=np.concatenate([singles['pair'], c['pair']]))
    moved, status, _ = case.fuse(30.0, c['rel'], **front)
    assert status == 0 and moved['members'][:5].tolist() == [1] * 5
    _same_bits(moved, whole, slice(5, None))
    assert np.array_equal(_bits(moved['x6d'][:5]), _bits(table[spare, 72:216].reshape(5, 24, 6)))
    behind = dict(table=table, order=np.concatenate([c['order'], spare, spare]), group=np.concatenate([c['group'], 100 + np.arange(10, dtype=np.int32)]),
                  pair=np.concatenate([c['pair'], singles['pair'], singles['pair']]))
    grown, status, _ = case.fuse(30.0, c['rel'], **behind)
    assert status == 0
    _same_bits(grown, whole, slice(0, vc.M))
    grown_part, status, _ = case.fuse(30.0, c['rel'], begin=0, count=vc.M, **behind)
    _same_bits(grown_part, whole, slice(0, vc.M))


def test_acc_is_a_function_of_the_multiset_of_positions(case):
    c = case.c
    whole, _ = case.accumulate()
    part, s1 = case.accumulate(begin=0, count=29)
    assert not torch.equal(part, whole)
    both, s2 = case.accumulate(begin=29, count=vc.M - 29, acc=part)
    assert s1 == 0 and s2 == 0 and torch.equal(both, whole)
    # the groups in another order (the blocks of positions permuted; a group's members stay in camera order)
    rng = np.random.RandomState(0)
    starts = np.nonzero(np.diff(c['group'], prepend=-1))[0]
    blocks = [np.arange(s, s + vc.GROUP_SIZES[g]) for g, s in enumerate(starts)]
    perm = np.concatenate([blocks[g] for g in rng.permutation(len(blocks))])
    assert (np.diff(c['group'][perm]) < 0).any()
    moved, status = case.accumulate(order=c['order'][perm], group=c['group'][perm], pair=c['pair'][perm])
    assert status == 0 and torch.equal(moved, whole)


def test_outputs_stay_inside_their_arrays_and_argument_errors_touch_nothing(case):
    c = case.c
    lib_mod = _mod('_lib')
    lib, ptr = lib_mod.load(), lib_mod.ptr
    sizes = (vc.M * 144, vc.M * 10, vc.M, vc.M, vc.M, vc.M)
    dtypes = (torch.float32,) * 4 + (torch.int32,) * 2
    bufs = [torch.full((n + 32,), 7, dtype=dt, device=DEV) for n, dt in zip(sizes, dtypes)]
    outs = [b[16:16 + n] for b, n in zip(bufs, sizes)]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    rel = T(c['rel']).to(DEV)
    d = case.dev
    acc = torch.full((case.n_pairs, vc.ACC_ROW), 7, dtype=torch.int64, device=DEV)
    stream = lib_mod.stream_ptr(d['table'].device)

    def fuse(begin, count, x6d=outs[0], table=d['table'], rel_=rel):
        return lib.jrr_view_fuse(ptr(table) if table is not None else None, vc.N_ROWS, ptr(d['order']), ptr(d['group']), ptr(d['pair']),
                                 ptr(rel_) if rel_ is not None else None, case.n_pairs, vc.M, vc.cos_half(30.0), begin, count,
                                 ptr(x6d) if x6d is not None else None, ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), ptr(outs[4]), ptr(outs[5]),
                                 ptr(status), stream)

    def relrot(acc_=acc, order=d['order'], count=vc.M):
        return lib.jrr_view_relrot_accumulate(ptr(d['table']), vc.N_ROWS, ptr(order) if order is not None else None, ptr(d['group']), ptr(d['pair']),
                                              ptr(d['ref_pair']), case.n_pairs, vc.M, 0, count, ptr(acc_) if acc_ is not None else None,
                                              ptr(status), stream)
    # misaligned or NULL arguments and a range outside the lists: JRR_ERR_ARG, nothing is touched
    assert fuse(0, vc.M, x6d=bufs[0][17:17 + sizes[0]]) == -1 and fuse(0, vc.M, x6d=None) == -1 and fuse(0, vc.M, table=None) == -1
    assert fuse(0, vc.M, rel_=None) == -1 and fuse(0, vc.M, table=d['table'].view(-1)[1:]) == -1 and fuse(3, vc.M - 2) == -1
    assert relrot(acc_=None) == -1 and relrot(order=None) == -1 and relrot(count=vc.M + 1) == -1
    assert relrot(acc_=acc.view(-1).view(torch.int32)[1:]) == -1                   # 4 bytes off: a misaligned int64 table
    torch.cuda.synchronize()
    assert all((b == 7).all().item() for b in bufs) and (acc == 7).all().item() and int(status.item()) == 0
    # a position range: the rows outside it and the guard words on either side keep their values
    begin, count = 3, 41
    lib_mod.check(fuse(begin, count), 'view_fuse')
    torch.cuda.synchronize()
    whole, _, _ = case.fuse(30.0, c['rel'])
    for b, o, name, per in zip(bufs, outs, NAMES, (144, 10, 1, 1, 1, 1)):
        assert (b[:16] == 7).all().item() and (b[-16:] == 7).all().item()
        o = o.cpu().numpy().reshape(vc.M, per)
        assert (o[:begin] == 7).all() and (o[begin + count:] == 7).all()
        assert np.array_equal(_bits(o[begin:begin + count]), _bits(whole[name].reshape(vc.M, per)[begin:begin + count])), name
    assert int(status.item()) == 0


# ---- 3. the status word ----
def _refused_checks(case, skipped, want_status, **kw):
    """positions that raise a bit: NaN / 0 outputs, nobody's members; everything else as the restatement has it, other groups' bits
    untouched; the accumulation reports the same bit"""
    c = case.c
    lists = {k: kw.get(k, c[k]) for k in ('table', 'order', 'group', 'pair')}
    valid, bits = vc.valid_positions(lists['table'], lists['order'], lists['group'], lists['pair'], case.n_pairs)
    assert bits == want_status and np.nonzero(~valid)[0].tolist() == sorted(skipped)
    got, status, _ = case.fuse(30.0, c['rel'], **kw)
    assert status == want_status
    x6d, betas = vc.positions_of(lists['table'], np.clip(lists['order'], 0, vc.N_ROWS - 1))
    want, d, _ = vc.yardstick(x6d, betas, lists['group'], np.minimum(lists['pair'], case.n_pairs - 1), c['rel'], 30.0, valid)
    _check_against(got, want, d, f'status {want_status}')
    for k in NAMES[:4]:
        assert np.isnan(got[k][skipped]).all(), k
    assert not got['members'][skipped].any() and not got['dropped'][skipped].any()
    clean, _, _ = case.fuse(30.0, c['rel'])
    far = ~np.isin(c['group'], c['group'][skipped]) & ~np.isin(lists['group'], lists['group'][skipped])
    _same_bits(got, clean, far, far)
    acc, status_acc = case.accumulate(**kw)
    assert status_acc == want_status
    count64 = vc.accumulate(x6d, lists['group'], np.minimum(lists['pair'], case.n_pairs - 1), c['ref_pair'], valid=valid)[0]
    assert np.array_equal(acc.cpu().numpy()[:, 0], count64)


def test_status_index_for_an_order_entry_outside_the_table(case):
    order = case.c['order'].copy()
    order[12], order[45] = vc.N_ROWS, -1
    _refused_checks(case, [12, 45], vc.STATUS_INDEX, order=order)


def test_status_marker_for_a_listed_row_without_marker(case):
    table = case.c['table'].copy()
    table[case.c['order'][37], 229] = 0.0
    table[case.c['order'][5], 229] = np.nan                                        # a marker that is not 1.0f, whatever else it is
    _refused_checks(case, [5, 37], vc.STATUS_MARKER, table=table)


def test_status_wide_for_a_group_of_nine(case):
    group = case.c['group'].copy()
    assert (group[10:18] == 4).all() and group[18] == 5
    group[18] = 4                                                                   # positions 10 .. 18: nine members
    _refused_checks(case, [10, 18], vc.STATUS_WIDE, group=group)


def test_status_pair_for_a_pair_id_beyond_n_pairs(case):
    pair = case.c['pair'].copy()
    pair[22], pair[50] = 9, 1 << 20
    _refused_checks(case, [22, 50], vc.STATUS_PAIR, pair=pair)
    order = case.c['order'].copy()
    order[0] = 1 << 20
    assert case.fuse(30.0, case.c['rel'], order=order, pair=pair)[1] == vc.STATUS_PAIR | vc.STATUS_INDEX


# ---- 4. planted truth ----
def test_planted_truth():
    """200 frames x 4 cameras, rotation noise |N(0, 5 deg)| per (frame, view, joint); the float64 restatement gives, for this seed:
    relative rotations 0.34, 0.37, 0.56 degrees from the planted ones (limit 1.5); mean body-rotation error 4.00 deg single -> 2.23 deg
    fused (ratio 0.558, limit 0.65); with view 2 replaced by a random rotation at 30 % of the (frame, joint) pairs, on those pairs 2.62 deg
    trimmed at 30 degrees against 3.98 deg for a clean single view and 26.1 deg for the plain mean; the replaced view dropped in 96.6 %."""
    refined = _mod('refined')
    ref = vc.planted_reference()                                                    # the case builder's own assertions, in float64
    clean = Case(vc.planted_case())
    c = clean.c
    acc, status = clean.accumulate()
    assert status == 0
    rel, residual = refined.relative_rotations(acc.cpu().numpy(), c['ref_pair'])
    count, mean = vc.acc_mean(acc.cpu().numpy())
    count64, mean64 = vc.accumulate(c['x6d'], c['group'], c['pair'], c['ref_pair'])
    d_acc = vc.dist(vc.accumulate(c['x6d'], c['group'], c['pair'], c['ref_pair'], F)[1], mean64)
    d_rel = np.abs(vc.solve(count64, vc.accumulate(c['x6d'], c['group'], c['pair'], c['ref_pair'], F)[1], c['ref_pair'])[0].astype(np.float64)
                   - ref['rel']).max()
    g_acc, g_rel = vc.dist(mean, mean64), np.abs(rel.astype(np.float64) - ref['rel']).max()
    print(f'acc {g_acc:.3e} (bound {vc.bound(d_acc):.3e}); d_c {g_rel:.3e} (yardstick {d_rel:.3e}, bound {vc.bound(d_rel):.3e})')
    assert np.array_equal(count, count64) and g_acc <= vc.bound(d_acc) and g_rel <= vc.bound(d_rel)
    truth = vc.planted_rel(c['E'], np.ones(4, bool)).astype(np.float64)
    err = np.degrees(2 * np.arccos(np.clip(np.abs(vc.qdot(rel.astype(np.float64), truth)), 0, 1)))
    print('relative rotations from the planted ones [deg]', err.round(3), 'residual', residual.round(2))
    assert err.max() <= 3 * 5.0 * np.sqrt(2.0 / 200) and abs(3 * 5.0 * np.sqrt(2.0 / 200) - 1.5) < 1e-12
    got, status, _ = clean.fuse(30.0, rel)
    e = vc.planted_errors(c, got['x6d'])
    print('clean', e, 'restatement', ref['clean'])
    assert status == 0 and e['fused'] <= 0.65 * e['single']
    # the orientation, fused in the reference camera's frame and taken back: closer to E_c W_0 than the single views are
    G, V = vc.PLANTED['frames'], vc.PLANTED['cams']
    W0 = c['E'][None] @ c['W'][:, None, 0]
    single0 = vc.rot_angle_deg(vc.rot6d(c['x6d'][:, 0]).reshape(G, V, 3, 3), W0).mean()
    fused0 = vc.rot_angle_deg(vc.rot6d(got['x6d'][:, 0]).reshape(G, V, 3, 3), W0).mean()
    print(f'orientation error {single0:.3f} -> {fused0:.3f} deg')
    assert fused0 <= 0.75 * single0
    bad = Case(vc.planted_case(replaced=True))
    trimmed, status, _ = bad.fuse(30.0, rel)
    t = vc.planted_errors(bad.c, trimmed['x6d'], trimmed['dropped'])
    plain, _, _ = bad.fuse(0.0, rel)
    p = vc.planted_errors(bad.c, plain['x6d'], plain['dropped'])
    print('replaced, 30 deg', t, '\nreplaced, plain mean', p)
    assert status == 0 and t['fused_bad'] <= t['single_clean'] and not p['fused_bad'] <= p['single_clean']
    assert t['flagged'] >= 0.95 and not plain['dropped'].any()


# ---- 5. through the driver's files ----
def _rig_dataset(root, smpl_model_np, j_h36m_np, n=40):
    """the dataset directory of view_fuse_cases.rig_dataset, written the way the time-axis tests write theirs"""
    sm = _mod('smpl_model')
    full = sm.synthetic_batch(smpl_model_np, j_h36m_np, n, seed=0)
    paths, orient, pose = vc.rig_dataset()
    d = os.path.join(root, 'precomputed_val')
    os.makedirs(d)
    tensors = {'bboxes': torch.tensor([[100., 200., 700., 800.]]).repeat(n, 1), 'betas': T(full['betas']),
               'estimated_translation': T(full['cam']), 'gt_j2d': torch.rand(n, 17, 2) * 1000, 'gt_j3d': T(full['gt_j3d']),
               'intrinsics': torch.eye(3).repeat(n, 1, 1), 'orient': T(orient), 'pose': T(pose)}
    for k, v in tensors.items():
        torch.save(v, os.path.join(d, f'{k}.pt'))
    with open(os.path.join(d, 'images.pkl'), 'wb') as f:
        pickle.dump(paths, f)
    return paths, full


def _with_args(flags, fn):
    argsmod = _mod('args')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(flags + ['--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent'])
    try:
        torch.manual_seed(0)
        return fn()
    finally:
        argsmod._LazyArgs._ns = saved


@pytest.fixture(scope='module')
def driver_table(tmp_path_factory, smpl_model_np, j_h36m_np):
    """a table the driver wrote from the 40-sample dataset directory (batches of 24: a shuffled loader, a ragged second batch)"""
    root = str(tmp_path_factory.mktemp('fuse_data'))
    paths, full = _rig_dataset(root, smpl_model_np, j_h36m_np)
    out_dir = os.path.join(root, 'refined')
    flags = ['--batch_size', '24', '--inner_iters', '2', '--device', DEV, '--synthetic', '--data_root', root]
    _with_args(flags + ['--save_refined', out_dir], lambda: _mod('optimize').optimize_pose_refiner(log=lambda r: None))
    return root, out_dir, paths, full, flags


def _check_fused_files(out_dir, paths, out, max_deg, source='refined.npz'):
    refined, eng = _mod('refined'), _mod('engine')
    raw = refined.load(out_dir, n=40, name=source)
    assert raw['has_refined'].all()
    order, group, pair, ref_pair, names, duplicates = refined.view_groups(paths, raw['has_refined'])
    assert np.bincount(group).tolist() == [4, 4, 4, 4, 1, 4, 3, 4, 4, 3, 4, 1] and duplicates == 0 and len(names) == 8
    back = refined.load(out_dir, n=40, name='refined_fused.npz')
    for k in ('pose', 'pose6d', 'shape', 'cam', 'view_group', 'n_views', 'view_pair', 'fuse_delta_body_deg', 'fuse_delta_orient_deg', 'fuse_dropped'):
        assert np.array_equal(back[k], out[k], equal_nan=True), k
    x6d, betas = raw['pose6d'][order], raw['shape'][order]
    count, mean = vc.accumulate(x6d, group, pair, ref_pair)
    rel = vc.solve(count, mean, ref_pair)[0]
    want, d, _ = vc.yardstick(x6d, betas, group, pair, rel, max_deg)                 # asserts the branch conditions on the file's rows
    got = {'x6d': back['pose6d'][order], 'betas': back['shape'][order], 'body': back['fuse_delta_body_deg'][order],
           'orient': back['fuse_delta_orient_deg'][order], 'members': back['n_views'][order], 'dropped': back['fuse_dropped'][order]}
    _check_against(got, want, d, f'files ({source})')
    # the fused `pose` is the log map of the fused `pose6d`: through batch_rodrigues it gives those matrices
    R = eng.rot6d_forward(T(back['pose6d']).to(DEV).reshape(-1, 6))
    d_rt = rc.yardsticks(R.cpu().numpy())[3]
    g_rt = float((eng.rodrigues_forward(T(back['pose']).to(DEV).reshape(-1, 3)) - R).abs().max().item())
    print(f'pose -> R against rot6d_forward(pose6d): {g_rt:.3e} (bound {rc.bound(d_rt):.3e})')
    assert g_rt <= rc.bound(d_rt)
    assert np.array_equal(_bits(back['cam']), _bits(raw['cam']))                    # cam belongs to the view
    for name in refined.EXTRA_NAMES + ('mpjpe_mm', 'pampjpe_mm', 'has_refined'):
        assert np.array_equal(back[name], raw[name], equal_nan=True), name
    assert np.array_equal(back['view_group'][order], group) and np.array_equal(back['view_pair'][order], pair)
    s = back['meta']['fuse']
    assert s['positions'] == 40 and s['groups'] == 12 and s['duplicates'] == 0 and s['max_deg'] == max_deg
    assert s['views_per_group_histogram'] == {'1': 2, '3': 2, '4': 8}
    assert [(p['scene'], p['camera']) for p in s['pairs']] == [tuple(n) for n in names]
    assert [p['count'] for p in s['pairs']] == count.tolist() and [p['reference'] for p in s['pairs']] == (ref_pair == np.arange(8)).tolist()
    print(f"moved body {s['fuse_delta_body_deg_mean']:.3f} deg, orientation {s['fuse_delta_orient_deg_mean']:.3f} deg, dropped {s['dropped_share']:.4f}; "
          f"residuals {[p['residual_deg'] and round(p['residual_deg'], 2) for p in s['pairs']]}")
    return raw, back


def test_fuse_views_on_a_table_the_driver_wrote(driver_table):
    root, out_dir, paths, full, flags = driver_table
    refined = _mod('refined')
    raw_bytes = open(os.path.join(out_dir, 'refined.npz'), 'rb').read()
    out = refined.fuse_views(out_dir, paths, max_deg=30.0, device=DEV)
    assert open(os.path.join(out_dir, 'refined.npz'), 'rb').read() == raw_bytes
    raw, back = _check_fused_files(out_dir, paths, out, 30.0)
    # the fused file feeds a run: it starts from those bits
    again = _with_args(flags[:2] + ['--inner_iters', '0'] + flags[4:] + ['--init_refined', os.path.join(out_dir, 'refined_fused.npz')],
                       lambda: _mod('optimize').optimize_pose_refiner(log=lambda r: None))
    idx = again['index'].numpy()
    assert np.array_equal(again['x6d'].cpu().numpy(), back['pose6d'][idx]) and np.array_equal(again['betas'].cpu().numpy(), back['shape'][idx])


def test_the_fuse_refined_command_with_its_re_evaluation(driver_table):
    root, out_dir, paths, full, flags = driver_table
    refined = _mod('refined')
    common = ['--data_root', root, '--synthetic', '--device', DEV, '--batch_size', '24']
    lines = []
    out = _with_args(['--fuse_refined', out_dir] + common, lambda: refined.fuse_command(log=lines.append))
    raw, back = _check_fused_files(out_dir, paths, out, 30.0)
    assert len(lines) == 1 and lines[0].startswith('fused 40 poses in 12 groups over 8 cameras (max 30 deg, 0 duplicates): body moved ')
    assert 'MPJPE' in lines[0] and lines[0].endswith(os.path.join(out_dir, 'refined_fused.npz'))
    print(lines[0])
    s = back['meta']['fuse']
    names = ('mpjpe_eval_mm_raw', 'pampjpe_eval_mm_raw', 'mpjpe_eval_mm_fused', 'pampjpe_eval_mm_fused')
    for name in names:
        assert back[name].shape == (40,) and back[name].dtype == F and np.array_equal(np.isfinite(back[name]), back['has_refined'] == 1)
        np.testing.assert_allclose(s[name + '_mean'], back[name].astype(np.float64).mean(), rtol=1e-12)
        assert f'{s[name + "_mean"]:.4f}' in lines[0]
    assert 'mpjpe_eval_mm_smooth' not in back
    # ... and on the smoothed table, by its name: the time-axis arrays travel along, the plain mean is one flag away
    _with_args(['--smooth_refined', out_dir] + common, lambda: refined.smooth_command(log=lambda s: None))
    out = _with_args(['--fuse_refined', os.path.join(out_dir, 'refined_smooth.npz'), '--fuse_max_deg', '0'] + common,
                     lambda: refined.fuse_command(log=lines.append))
    assert len(lines) == 2 and '(max 0 deg' in lines[1] and not out['fuse_dropped'].any()
    back = refined.load(out_dir, n=40, name='refined_fused.npz')
    smooth = refined.load(out_dir, n=40, name='refined_smooth.npz')
    for name in ('jitter_deg', 'run_id', 'mpjpe_eval_mm_smooth'):
        assert np.array_equal(back[name], smooth[name], equal_nan=True), name
    assert not np.array_equal(back['pose6d'], smooth['pose6d']) and np.array_equal(_bits(back['cam']), _bits(smooth['cam']))
    for name in names:
        assert np.isfinite(back[name]).all()
    assert 'smooth' in back['meta'] and back['meta']['fuse']['max_deg'] == 0.0
    # one process: another rank returns at once
    os.environ['RANK'] = '1'
    try:
        assert _with_args(['--fuse_refined', out_dir, '--data_root', root], lambda: refined.fuse_command(log=lines.append)) is None
    finally:
        del os.environ['RANK']
    assert len(lines) == 2
