"""The per-vertex error on the GPU (pytest -m gpu): jrr_vertex_error against float64 and the reference's stored values
(tests/golden/g12_vertex_error.npz), the properties include/jrr.h promises, `--eval_pve` through the mesh evaluation and
tools/dump_eval_vertices.py --gt_refined.

Bounds (vertex_error_cases.bound): max(floor, 1.5 x the float32 restatement's distance from float64 on the SAME
inputs); the floors are the reference's own float32 distance from float64 on the fixture's families as tests/golden/make_golden_pve.py
printed it, rounded up to one digit: 2e-6 m per vertex, 4e-7 m per pose.  Against the stored values of the reference the kernel may
be its bound plus the reference's own distance (the floor) away: both are measured from float64.  The tables are held EXACTLY to the
host-side integer accumulation of the float32 values the same call wrote.

Shapes: 1, 3, 63, 64, 65, 255, 256, 257 and 431 vertices around the wave and the 256-thread workgroup, 6890 (the body), 7168 and 7169
(the last size whose vertices a workgroup keeps in registers and whose per-vertex table it sums in LDS, and the first that reads the
meshes again and adds per pose); batches 1, 2, 5 and 70; 300 poses where a workgroup owns more than one."""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest
import torch

import eval_report_cases as ec
import vertex_error_cases as vc
from conftest import PKG_NAME, ROOT, load_golden

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
F, F64 = np.float32, np.float64
VERTS = (1, 3, 63, 64, 65, 255, 256, 257, 431, 6890, 7168, 7169)
BATCHES = (1, 2, 5, 70)


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(*arrays):
    return [None if a is None else T(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _call(pred, gt, rp=None, rg=None, **kw):
    """engine.vertex_error on numpy inputs -> numpy outputs (None stays None)"""
    p, q, a, b = _dev(pred, gt, rp, rg)
    out = _mod('engine').vertex_error(p, q, a, b, **kw)
    return [None if t is None else t.cpu().numpy() for t in out]


def _tables(n_groups, n):
    return (torch.zeros(n_groups * vc.ROW + vc.TRAILER, dtype=torch.int64, device=DEV), torch.zeros(2, n, dtype=torch.int64, device=DEV))


# ---- 1. the values ----
@pytest.fixture(scope='module')
def references():
    """per vertex count: the 70 mixed poses, their float64 evaluation and the float32 restatement -- computed once, never changed"""
    cache = {}

    def get(n):
        if n not in cache:
            pred, gt, rp, rg, fam = vc.mixed_case(n, max(BATCHES))
            cache[n] = (pred, gt, rp, rg, fam, vc.evaluate64(pred, gt, rp, rg), vc.restate(pred, gt, rp, rg))
        return cache[n]
    return get


@pytest.mark.parametrize('n_verts', VERTS)
def test_values_against_float64(references, n_verts):
    pred, gt, rp, rg, fam, r64, r32 = references(n_verts)
    names = list(vc.FAMILIES)
    const_t = np.array([names[f] == 'constant_target' for f in fam])
    for B in BATCHES:
        pve, pa, d, e = _call(pred[:B], gt[:B], rp[:B], rg[:B])
        assert d.shape == (B, n_verts) and e.shape == (B, n_verts) and pve.shape == (B,) and all(a.dtype == F for a in (pve, pa, d, e))
        assert np.isfinite(d).all() and np.isfinite(pve).all()
        if n_verts == 1:
            assert np.isnan(e).all() and np.isnan(pa).all()                 # one vertex is a constant pred: NaN in the aligned values only
            assert vc.dist(d, r64[0][:B]) <= vc.FLOOR_VERTEX
            continue
        assert np.isfinite(e).all() and np.isfinite(pa).all()
        assert not e[const_t[:B]].any() and not pa[const_t[:B]].any()       # a constant target: exactly 0
        for what, got, k, floor in (('d', d, 0, vc.FLOOR_VERTEX), ('e', e, 1, vc.FLOOR_VERTEX), ('pve', pve, 2, vc.FLOOR_POSE), ('pa_pve', pa, 3, vc.FLOOR_POSE)):
            own = vc.dist(r32[k][:B], r64[k][:B])
            b, dist = vc.bound(own, floor), vc.dist(got, r64[k][:B])
            print(f'n_verts {n_verts} B {B} {what}: {dist:.3e} m from float64 (restatement {own:.3e}, bound {b:.3e}); '
                  f'bits equal to the restatement: {np.array_equal(_bits(got), _bits(r32[k][:B]))}')
            assert dist <= b
        # the means are the exact integer means of the distances the call wrote
        assert np.array_equal(_bits(pve), _bits(vc.pose_mean(d))) and np.array_equal(_bits(pa), _bits(vc.pose_mean(e)))


@pytest.mark.parametrize('n_verts', vc.G12_VERTS)
def test_values_against_the_references_stored_values(n_verts):
    g = load_golden('g12_vertex_error.npz')
    sub = vc.subset(n_verts)
    cases = [vc.family_case(name, n_verts) for name in vc.FAMILIES]
    pred, gt, rp, rg = (np.concatenate([c[k] for c in cases]) for k in range(4))
    pve, pa, d, e = _call(pred, gt, rp, rg)                                 # one launch of 20
    r64, r32 = vc.evaluate64(pred, gt, rp, rg), vc.restate(pred, gt, rp, rg)
    for i, name in enumerate(vc.FAMILIES):
        sl = slice(i * vc.G12_POSES, (i + 1) * vc.G12_POSES)
        for what, got, k, floor, stored in (('d', d[sl][:, sub], 0, vc.FLOOR_VERTEX, g[f'{name}_{n_verts}_d']), ('e', e[sl][:, sub], 1, vc.FLOOR_VERTEX, g[f'{name}_{n_verts}_e']),
                                            ('pve', pve[sl], 2, vc.FLOOR_POSE, g[f'{name}_{n_verts}_pve']), ('pa_pve', pa[sl], 3, vc.FLOOR_POSE, g[f'{name}_{n_verts}_pa'])):
            b = vc.bound(vc.dist(r32[k][sl], r64[k][sl]), floor)
            dist = vc.dist(got, stored)
            print(f'g12 {name} {n_verts} {what}: {dist:.3e} m from the stored values (bound {b:.3e} + floor {floor:.0e})')
            assert dist <= b + floor


def test_the_references_degenerate_poses_as_17_vertex_meshes():
    """tests/golden/g11_eval_degenerate.npz at n_verts = 17: target / 1000 formed on the host, roots = joint 0 -- the inputs of
    jrr_evaluate_joints; every family within the bound its stored values give, and a constant pred beside them"""
    g = load_golden('g11_eval_degenerate.npz')
    cp, ct = ec.family_cases('constant_pred', ec.G11_POSES)
    pred, tgt = np.concatenate([g['pred'], cp]), (np.concatenate([g['target_mm'], ct]) / F(1000)).astype(F)
    _, e64, pa64 = ec.evaluate_joints(pred, tgt * F64(1000), torch.float64)
    pve, pa, d, e = _call(pred, tgt, pred[:, 0].copy(), tgt[:, 0].copy())
    n = ec.G11_POSES
    for k, name in enumerate(ec.G11_FAMILIES):
        sl = slice(k * n, (k + 1) * n)
        d_plain, d_pa = vc.dist(g['err_j'][sl], e64[sl]), vc.dist(g['err_pa_j'][sl], pa64[sl])
        assert d_pa <= ec.FAMILIES[name][1]
        got = vc.dist(d[sl], e64[sl]), vc.dist(e[sl], pa64[sl]), vc.dist(d[sl], g['err_j'][sl]), vc.dist(e[sl], g['err_pa_j'][sl])
        print(f'g11 {name}: from float64 plain {got[0]:.3e} PA {got[1]:.3e}; from the stored values plain {got[2]:.3e} PA {got[3]:.3e} '
              f'(reference {d_plain:.3e} / {d_pa:.3e}, bounds {ec.bound(d_plain):.3e} / {ec.bound(d_pa):.3e})')
        assert got[0] <= ec.bound(d_plain) and got[2] <= ec.bound(d_plain) and got[1] <= ec.bound(d_pa) and got[3] <= ec.bound(d_pa)
        assert np.isfinite(e[sl]).all()
        if name == 'constant_target':
            assert not e[sl].any() and not pa[sl].any()
    last = slice(len(ec.G11_FAMILIES) * n, None)
    assert np.isnan(e[last]).all() and np.isnan(pa[last]).all() and np.isfinite(d[last]).all() and np.isfinite(pve[last]).all()
    assert vc.dist(d[last], e64[last]) <= vc.FLOOR_VERTEX


# ---- 2. what the header promises ----
@pytest.mark.parametrize('n_verts', (65, 6890, 7169))
def test_a_pose_does_not_depend_on_its_batch_or_its_place(references, n_verts):
    pred, gt, rp, rg, *_ = references(n_verts)
    whole = _call(pred, gt, rp, rg)
    alone = _call(pred[33:34], gt[33:34], rp[33:34], rg[33:34])
    order = np.random.RandomState(1).permutation(70)
    moved = _call(pred[order], gt[order], rp[order], rg[order])
    big = np.arange(300) % 70                                                # 300 poses: workgroups own more than one
    many = _call(pred[big], gt[big], rp[big], rg[big])
    for k in range(4):
        assert np.array_equal(_bits(whole[k][33:34]), _bits(alone[k]))
        assert np.array_equal(_bits(whole[k][order]), _bits(moved[k]))
        assert np.array_equal(_bits(whole[k][big]), _bits(many[k]))


@pytest.fixture(scope='module')
def table_case():
    """431 vertices, 70 poses in 3 groups: one pose ignored, one with a group outside, one with a NaN vertex, one constant pred
    (its aligned mean is NaN), parts with an empty one (label 2 never occurs) and an out-of-range label"""
    pred, gt, rp, rg, fam = vc.mixed_case(431, 70, seed=9)
    pred = pred.copy()
    pred[11, 100, 1] = np.nan
    pred[12] = pred[12, [5]]
    group = (np.arange(70) % 3).astype(np.int32)
    group[20], group[21] = -1, 3
    part = (np.arange(431) % 5).astype(np.int32)
    part[part == 2] = 4
    part[7], part[8] = 9, -1
    return pred, gt, rp, rg, group, part


def _table_call(case, sel=slice(None), group='case', n_groups=3, part='case', acc='new', **kw):
    pred, gt, rp, rg, g, p = case
    g = g if isinstance(group, str) else group
    p = p if isinstance(part, str) else part
    t, tv = _tables(n_groups, pred.shape[1]) if isinstance(acc, str) else acc
    gd, pd = _dev(None if g is None else g[sel], p)
    out = _call(pred[sel], gt[sel], rp[sel], rg[sel], group=gd, part=pd, n_parts=5 if p is not None else 0, n_groups=n_groups, acc=t, acc_v=tv, **kw)
    return out, t, tv


def test_tables_are_exactly_the_integer_accumulation_of_the_values_the_call_wrote(table_case):
    pred, gt, rp, rg, group, part = table_case
    (pve, pa, d, e), t, tv = _table_call(table_case)
    assert np.isnan(pve[11]) and np.isnan(pa[11]) and np.isfinite(pve[12]) and np.isnan(pa[12]) and int(np.isnan(d).sum()) == 1
    want, want_v = vc.accumulate(d, e, pve, pa, group, 3, part, 5)
    table, table_v = t.cpu().numpy(), tv.cpu().numpy()
    assert np.array_equal(table, want) and np.array_equal(table_v, want_v)
    rows = table[:-2].reshape(3, vc.ROW)
    assert table[-2:].tolist() == [1, 1] and int(rows[:, vc.COUNT].sum()) == 66 and int(rows[:, vc.BAD].sum()) == 2
    assert not rows[:, vc.PART + 2].any() and not rows[:, vc.PART + 5:vc.PART + 32].any() and rows[:, vc.PART:vc.PART + 2].all()
    counted = (group >= 0) & (group < 3) & ~np.isnan(pve) & ~np.isnan(pa)
    assert np.array_equal(table_v[0], vc.fixed(d[counted]).sum(0)) and int(table_v[0].min()) > 0
    # the derived numbers are the float64 means of the values, to their quantum
    doc = _mod('vertex_report').derive(np.concatenate([table[:-1], [0]]), table_v, ['a', 'b', 'c'], part, 5)
    assert abs(doc['all']['pve_mm'] - pve[counted].astype(F64).mean() * 1000) <= 1000 * 2.0 ** -25
    assert abs(doc['all']['pa_pve_mm'] - pa[counted].astype(F64).mean() * 1000) <= 1000 * 2.0 ** -25
    assert doc['all']['pve_per_part_mm']['R_Hip'] is None and doc['ignored'] == 1
    assert abs(doc['all']['pve_per_part_mm']['Pelvis'] - d[counted][:, part == 0].astype(F64).mean() * 1000) <= 1000 * 2.0 ** -24
    # no groups and no parts: everything in group 0, no part words, the trailer empty; the values are the same bits
    (pve0, pa0, d0, e0), t0, tv0 = _table_call(table_case, group=None, n_groups=1, part=None)
    w0, wv0 = vc.accumulate(d0, e0, pve0, pa0, None, 1)
    assert np.array_equal(t0.cpu().numpy(), w0) and np.array_equal(tv0.cpu().numpy(), wv0) and w0[-2:].tolist() == [0, 0] and int(w0[vc.COUNT]) == 68
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip((pve0, pa0, d0, e0), (pve, pa, d, e)))


def test_split_calls_a_permuted_batch_and_many_poses_per_workgroup_give_the_same_tables(table_case):
    _, t, tv = _table_call(table_case, means=False, rows=False)
    acc = _tables(3, 431)
    for sl in (slice(0, 31), slice(31, 70)):                                # two calls add into one pair of tables
        _table_call(table_case, sel=sl, acc=acc, means=False, rows=False)
    assert torch.equal(acc[0], t) and torch.equal(acc[1], tv)
    order = np.random.RandomState(2).permutation(70)
    _, tp, tvp = _table_call(table_case, sel=order, means=False, rows=False)
    assert torch.equal(tp, t) and torch.equal(tvp, tv)
    rep = np.arange(350) % 70                                               # 350 poses on 256 workgroups: the LDS sums cover two poses
    _, t5, tv5 = _table_call(table_case, sel=rep, means=False, rows=False)
    assert torch.equal(t5, 5 * t) and torch.equal(tv5, 5 * tv)


@pytest.mark.parametrize('n_verts', (7168, 7169))
def test_per_vertex_table_on_both_sides_of_the_register_threshold(references, n_verts):
    pred, gt, rp, rg, *_ = references(n_verts)
    t, tv = _tables(2, n_verts)
    group = (np.arange(5) % 2).astype(np.int32)
    part = (np.arange(n_verts) % 24).astype(np.int32)
    gd, pd = _dev(group, part)
    pve, pa, d, e = _call(pred[:5], gt[:5], rp[:5], rg[:5], group=gd, part=pd, n_parts=24, n_groups=2, acc=t, acc_v=tv)
    want, want_v = vc.accumulate(d, e, pve, pa, group, 2, part, 24)
    assert np.array_equal(t.cpu().numpy(), want) and np.array_equal(tv.cpu().numpy(), want_v) and int(want_v.min()) >= 0 and want_v[0].all()


def test_a_nan_vertex_adds_bad_only_and_groups_outside_reach_the_trailer_only(table_case):
    pred, gt, rp, rg, group, part = table_case
    for row, word in ((11, vc.BAD), (12, vc.BAD)):
        _, t, tv = _table_call(table_case, sel=slice(row, row + 1))
        table = t.cpu().numpy()
        assert int(table[int(group[row]) * vc.ROW + word]) == 1 and int(np.abs(table).sum()) == 1 and not tv.any()
    for row, word in ((20, 0), (21, 1)):
        _, t, tv = _table_call(table_case, sel=slice(row, row + 1))
        table = t.cpu().numpy()
        assert int(table[3 * vc.ROW + word]) == 1 and int(np.abs(table).sum()) == 1 and not tv.any()


# ---- 3. outputs alone, an empty batch, refused arguments ----
def test_each_output_alone_and_an_empty_batch(table_case):
    eng = _mod('engine')
    pred, gt, rp, rg, group, part = table_case
    p, q, a, b, gd, pd = _dev(pred, gt, rp, rg, group, part)
    (pve, pa, d, e), t, tv = _table_call(table_case)
    lib, ptr = _mod('_lib').load(), _mod('_lib').ptr
    s = _mod('_lib').stream_ptr(torch.device(DEV))

    def raw(pve_=None, pa_=None, d_=None, e_=None, acc_=None, accv_=None, batch=70):
        return lib.jrr_vertex_error(ptr(p), ptr(q), ptr(a), ptr(b), ptr(gd), ptr(pd), 5, batch, 431, 3, ptr(pve_), ptr(pa_), ptr(d_), ptr(e_), ptr(acc_),
                                    ptr(accv_), s)
    for k, (want, shape) in enumerate(((pve, (70,)), (pa, (70,)), (d, (70, 431)), (e, (70, 431)))):
        out = torch.full(shape, -1.0, device=DEV)
        assert raw(**{('pve_', 'pa_', 'd_', 'e_')[k]: out}) == 0
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    t1, tv1 = _tables(3, 431)
    assert raw(acc_=t1) == 0 and torch.equal(t1, t)
    assert raw(accv_=tv1) == 0 and torch.equal(tv1, tv)
    # an empty batch: JRR_OK, nothing touched
    out = torch.full((70,), -1.0, device=DEV)
    t2, tv2 = _tables(3, 431)
    assert raw(pve_=out, acc_=t2, accv_=tv2, batch=0) == 0
    torch.cuda.synchronize()
    assert (out == -1).all() and not t2.any() and not tv2.any()
    assert eng.vertex_error(p[:0], q[:0])[0].shape == (0,)


def test_refused_arguments_leave_a_message_and_touch_nothing(table_case):
    pred, gt, rp, rg, group, part = table_case
    p, q, a, b, gd, pd = _dev(pred, gt, rp, rg, group, part)
    lib, ptr = _mod('_lib').load(), _mod('_lib').ptr
    s = _mod('_lib').stream_ptr(torch.device(DEV))
    out = [torch.full((70,), -1.0, device=DEV), torch.full((70,), -1.0, device=DEV), torch.full((70, 431), -1.0, device=DEV),
           torch.full((70, 431), -1.0, device=DEV)]
    t, tv = _tables(3, 431)
    t += 7
    tv += 7
    good = dict(pred=p, gt=q, rp=a, rg=b, group=gd, part=pd, n_parts=5, batch=70, n=431, n_groups=3, o=out, acc=t, accv=tv)

    def raw(**kw):
        k = dict(good, **kw)
        o = k['o']
        if 'off' in k:                                                       # an address that is not a multiple of the element size
            name, nbytes = k['off']
            shifted = ctypes.c_void_p(k[name].data_ptr() + nbytes)
            if name == 'acc':
                return lib.jrr_vertex_error(ptr(k['pred']), ptr(k['gt']), ptr(k['rp']), ptr(k['rg']), ptr(k['group']), ptr(k['part']), k['n_parts'],
                                            k['batch'], k['n'], k['n_groups'], ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), shifted, ptr(k['accv']), s)
            return lib.jrr_vertex_error(shifted, ptr(k['gt']), ptr(k['rp']), ptr(k['rg']), ptr(k['group']), ptr(k['part']), k['n_parts'], k['batch'],
                                        k['n'], k['n_groups'], ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), ptr(k['acc']), ptr(k['accv']), s)
        return lib.jrr_vertex_error(ptr(k['pred']), ptr(k['gt']), ptr(k['rp']), ptr(k['rg']), ptr(k['group']), ptr(k['part']), k['n_parts'], k['batch'],
                                    k['n'], k['n_groups'], ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), ptr(k['acc']), ptr(k['accv']), s)
    cases = [(dict(pred=None), 'pred and gt are required'), (dict(gt=None), 'pred and gt are required'),
             (dict(o=[None] * 4, acc=None, accv=None), 'no output'), (dict(batch=-1), 'batch must be >= 0'), (dict(n=0), 'n_verts in 1 .. 65536'),
             (dict(n=65537), 'n_verts in 1 .. 65536'), (dict(n_parts=0), 'n_parts must lie in 1 .. 32'), (dict(n_parts=33), 'n_parts must lie in 1 .. 32'),
             (dict(n_groups=0), 'n_groups 0: 1 .. 1024'), (dict(n_groups=1025), 'n_groups 1025: 1 .. 1024'),
             (dict(n_groups=0, acc=None), 'n_groups 0: 1 .. 1024'), (dict(off=('pred', 2)), '4-byte aligned'), (dict(off=('acc', 4)), '8-byte aligned')]
    for kw, msg in cases:
        assert raw(**kw) == -1, kw                                           # JRR_ERR_ARG
        text = lib.jrr_last_error().decode()
        assert text.startswith('jrr_vertex_error: ') and msg in text, (kw, text)
    torch.cuda.synchronize()
    assert all((o == -1).all() for o in out) and (t == 7).all() and (tv == 7).all()
    # n_groups is not looked at without a table that needs it
    assert raw(n_groups=0, acc=None, accv=None) == 0 and raw(n_groups=0, acc=None, group=None) == 0
    torch.cuda.synchronize()


# ---- 4. --eval_pve through the mesh evaluation ----
SYN = ['--synthetic', '--device', DEV, '--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent']


def _with_args(flags, fn):
    argsmod = _mod('args')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(flags)
    try:
        return fn()
    finally:
        argsmod._LazyArgs._ns = saved


def test_eval_pve_through_eval_vertices(tmp_path, smpl_model_np):
    """7 meshes of the synthetic body at --batch_size 3 (a ragged last chunk), two groups, one mesh ignored, one target with a NaN"""
    eng, sm, vr, er, utils = _mod('engine'), _mod('smpl_model'), _mod('vertex_report'), _mod('eval_report'), _mod('utils')
    tmp = str(tmp_path)
    J = sm.default_h36m_regressor()
    J2 = (J * (1 + 0.5 * np.random.RandomState(5).rand(*J.shape))).astype(F)
    ck = os.path.join(tmp, 'retrained_J_Regressor.pt')
    _mod('checkpoint').save_j_regressor(T(J2), ck)
    N = 7
    batch = sm.synthetic_batch(smpl_model_np, J, N, seed=123)
    e = eng.RefineEngine(eng.DeviceModel(smpl_model_np, DEV), N, flags=eng.FLAG_KEEP_VERTS)
    e.set_j_regressor(T(J).to(DEV), torch.ones(17, 6890, device=DEV))
    _, verts = e.find_joints_forward(T(batch['betas']).to(DEV), x6d=T(batch['pose6d']).to(DEV), return_verts=True)
    verts = verts.cpu().numpy()
    rs = np.random.RandomState(8)
    gt_verts = (verts * F(1.03) + rs.randn(N, 6890, 3) * 0.01 + rs.randn(N, 1, 3) * 0.2).astype(F)
    gt_verts[5, 1000, 2] = np.nan
    ids = np.array([0, 1, 0, 1, -1, 0, 1], dtype=np.int32)
    vdir = os.path.join(tmp, 'meshes')
    os.makedirs(vdir)
    np.save(os.path.join(vdir, 'vertices.npy'), verts)
    np.save(os.path.join(vdir, 'gt_vertices.npy'), gt_verts)
    np.save(os.path.join(vdir, 'gt_j3d.npy'), batch['gt_j3d'].astype(F))
    np.save(os.path.join(vdir, 'group.npy'), ids)
    with open(os.path.join(vdir, 'group_names.txt'), 'w') as f:
        f.write('SPIN\nVIBE\n')
    flags = SYN + ['--batch_size', '3', '--eval_j_regressor', ck, '--eval_vertices', vdir]
    plain, with_pve, lines = os.path.join(tmp, 'plain'), os.path.join(tmp, 'pve'), []
    _with_args(flags + ['--eval_report', plain], lambda: er.evaluate_vertices(log=lambda s: None))
    _with_args(flags + ['--eval_report', with_pve, '--eval_pve', '--eval_pve_parts'], lambda: er.evaluate_vertices(log=lines.append))
    assert sorted(os.listdir(plain)) == ['eval.json', 'eval.md'] and sorted(os.listdir(with_pve)) == ['eval.json', 'eval.md', 'pve.json', 'pve.md', 'pve_per_vertex.npy']
    a, b = er.load(plain), er.load(with_pve)
    assert a['regressors'] == b['regressors']                               # eval.json holds the same numbers
    assert {k: v for k, v in a['flags'].items() if k != 'eval_report'} == {k: v for k, v in b['flags'].items() if k != 'eval_report'}
    assert open(os.path.join(plain, 'eval.md'), encoding='utf-8').read() == open(os.path.join(with_pve, 'eval.md'), encoding='utf-8').read().replace(ck, ck)
    assert sum(line.startswith('per-vertex error, mm: PVE ') for line in lines) == 1
    # the direct call: joint 0 of the initial regressor with its mask centres both meshes; one launch of 7
    doc = vr.load(with_pve)
    dv, dq, di = _dev(verts, gt_verts, ids)
    table = eng.JointRegressorTable(T(J).to(DEV), utils.find_j_reg_mask(T(J)).to(DEV))
    part = vr.part_labels(smpl_model_np['lbs_weights'])
    t, tv = _tables(2, 6890)
    eng.vertex_error(dv, dq, table.regress(dv)[0][:, 0].contiguous(), table.regress(dq)[0][:, 0].contiguous(), group=di, part=T(part).to(DEV), n_parts=24,
                     n_groups=2, acc=t, acc_v=tv, means=False, rows=False)
    want = vr.derive(t.cpu().numpy(), tv.cpu().numpy(), ['SPIN', 'VIBE'], part, 24)
    per_vertex = np.load(os.path.join(with_pve, 'pve_per_vertex.npy'))
    assert per_vertex.shape == (2, 6890) and per_vertex.dtype == F and np.array_equal(per_vertex, want.pop('per_vertex_mm'))
    assert doc['data'] == json.loads(json.dumps(want)) and doc['groups'] == ['SPIN', 'VIBE'] and doc['n_verts'] == 6890
    assert doc['data']['all']['n'] == 5 and doc['data']['all']['n_bad'] == 1 and doc['data']['ignored'] == 1
    assert 0 < doc['data']['all']['pa_pve_mm'] < doc['data']['all']['pve_mm'] and len(doc['data']['all']['pve_per_part_mm']) == 24
    md = open(os.path.join(with_pve, 'pve.md'), encoding='utf-8').read()
    assert '| SPIN | 2 | 1 |' in md and '| VIBE | 3 | 0 |' in md and '| all | 5 | 1 |' in md and '| Pelvis |' in md


# ---- 5. tools/dump_eval_vertices.py --gt_refined ----
def test_dump_eval_vertices_writes_the_refined_meshes(smpl_model_np, j_h36m_np, tmp_path):
    """the dataset stand-in of test_gpu_refined_export.py::test_driver_on_a_dataset_then_init_refined (40 samples, batches of 24),
    --save_refined, then the tool with --gt_refined on a table whose rows 3 and 30 hold no refined pose"""
    sm, refined, eng = _mod('smpl_model'), _mod('refined'), _mod('engine')
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
    flags = ['--batch_size', '24', '--inner_iters', '2', '--device', DEV, '--synthetic', '--data_root', str(tmp_path), '--smpl_dir', '/nonexistent',
             '--j_regressor_init', '/nonexistent']
    out_dir = str(tmp_path / 'refined')
    _with_args(flags + ['--save_refined', out_dir], lambda: (torch.manual_seed(0), _mod('optimize').optimize_pose_refiner(log=lambda r: None)))
    arr = refined.load(out_dir, n=n)
    assert arr['has_refined'].tolist() == [1] * n
    # a second table in which two rows hold no refined pose
    holes = {k: v.copy() for k, v in arr.items() if k != 'meta'}
    holes['has_refined'][[3, 30]] = 0
    np.savez(os.path.join(out_dir, 'holes.npz'), **holes)
    import pickle
    paths = [f'/data/h36m/S9/Walking 1/imageSequence/1/img_{5 * (i + 1):06d}.jpg' for i in range(n)]
    with open(str(d / 'images.pkl'), 'wb') as f:                            # written after the driver ran: the tool alone reads it
        pickle.dump(paths, f)
    import importlib.util
    spec = importlib.util.spec_from_file_location('dump_eval_vertices', os.path.join(ROOT, 'tools', 'dump_eval_vertices.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    saved = _mod('args')._LazyArgs._ns
    try:
        tool.main([str(tmp_path / 'plain')] + flags)
        tool.main([str(tmp_path / 'gt'), '--gt_refined', os.path.join(out_dir, 'holes.npz')] + flags)
    finally:
        _mod('args')._LazyArgs._ns = saved
    assert sorted(os.listdir(str(tmp_path / 'plain'))) == ['gt_j3d.npy', 'paths.txt', 'vertices.npy']      # without the flag: what it wrote before
    v0, j0 = np.load(str(tmp_path / 'plain' / 'vertices.npy')), np.load(str(tmp_path / 'plain' / 'gt_j3d.npy'))
    v, gv, gj = (np.load(str(tmp_path / 'gt' / f)) for f in ('vertices.npy', 'gt_vertices.npy', 'gt_j3d.npy'))
    assert v0.shape == (24, 6890, 3)                                        # drop_last: one batch of 24 of the 40
    # the batch's dataset rows, from the ground truth the dataset holds; the tool keeps those with a refined pose, in order, in every file
    rows = [int(np.flatnonzero((full['gt_j3d'].astype(F) == j).all((1, 2)))[0]) for j in j0]
    assert len(set(rows)) == 24
    keep = [k for k, r in enumerate(rows) if r not in (3, 30)]
    m = len(keep)
    assert v.shape == (m, 6890, 3) and gv.shape == (m, 6890, 3) and gj.shape == (m, 17, 3) and gv.dtype == F
    assert np.array_equal(v, v0[keep]) and np.array_equal(gj, j0[keep])
    with open(str(tmp_path / 'gt' / 'paths.txt')) as f:
        assert [line.rstrip('\n') for line in f] == [paths[rows[k]] for k in keep]
    # gt_vertices.npy: the engine's forward of the table's rows (the tool's own launch: the batch of 24)
    e = eng.RefineEngine(eng.DeviceModel(smpl_model_np, DEV), 24, flags=eng.FLAG_KEEP_VERTS)
    e.set_j_regressor(T(sm.default_h36m_regressor()).to(DEV))
    _, want = e.find_joints_forward(T(arr['shape'][rows]).to(DEV).contiguous(), x6d=T(arr['pose6d'][rows]).to(DEV).contiguous(), return_verts=True)
    assert np.array_equal(gv, want.cpu().numpy()[keep])
    assert not np.array_equal(gv, v)                                        # the refined poses are not the dataset's
