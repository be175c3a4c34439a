"""`--place_refined` on the GPU (pytest -m gpu): jrr_place_translation against the float64 host restatement (tests/place_cases.py),
jrr_project_points against float64, jrr_place_accumulate word for word against the integer accumulation of the kernel's own outputs, the
refusals of the three entry points, and the command end to end on a split whose pixels were made from planted translations.

Bounds, as the issue sets them: `trans` within 1e-7 m of the restatement (both sides are fp64 in the same order; they may differ by
the device's sqrt and by accept / reject decisions of steps below 1e-9 m), `status` equal, `err` / `err_lin` within 1e-3 px (fp32
storage of values up to ~1e3), NaN exactly where the restatement has it; the projection within 16 x 2^-24 x (|f X / Z| + |c|) of
float64 arithmetic on the same float32 inputs (five roundings with threefold slack).

Shapes: a pool of 1000 poses with the four refusals inside, at batches 1, 2, 63, 64, 65, 257 and 1000 (one pose, a partial wave, the
edges of a wave -- which is a workgroup here -- and many workgroups) and 0, 1 and 10 steps, written inside frames of sentinel values.
"""
import ctypes
import importlib
import json
import os
import pickle

import numpy as np
import pytest
import torch

import place_cases as pc
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
F, F64 = np.float32, np.float64
SENTINEL = -7.0


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _dev(a):
    return None if a is None else T(np.ascontiguousarray(a)).to(DEV)


def _run(joints, j2d, K, weight, n_iters, want_linear=True):
    """jrr_place_translation on host arrays, every output inside a frame of sentinels: (trans, err_lin, err, status) on the host"""
    B = joints.shape[0]
    frames = [torch.full((B + 2, 3), SENTINEL, dtype=torch.float64, device=DEV), torch.full((B + 2, 17), SENTINEL, device=DEV),
              torch.full((B + 2, 17), SENTINEL, device=DEV), torch.full((B + 2,), -99, dtype=torch.int32, device=DEV)]
    out = [f[1:B + 1] for f in frames]
    if not want_linear:
        out[1] = None
    _mod('engine').place_translation(_dev(joints), _dev(j2d), _dev(K), _dev(weight), n_iters, out=tuple(out))
    host = [f.cpu().numpy() for f in frames]
    for k, h in enumerate(host):
        fill = -99 if k == 3 else SENTINEL
        assert (h[0] == fill).all() and (h[B + 1] == fill).all()
    if not want_linear:
        assert (host[1] == SENTINEL).all()
    return tuple(h[1:B + 1].copy() for h in host)


class Pool:
    """place_cases.gpu_pool with what the restatement says about it at every step count (computed once, never changed)"""

    def __init__(self):
        self.joints, self.j2d, self.K, self.weight, self.planted, self.regular = pc.gpu_pool()
        self.ref = {n: pc.place(self.joints, self.j2d, self.K, self.weight, n) for n in pc.GPU_ITERS}
        self.whole = _run(self.joints, self.j2d, self.K, self.weight, 10)

    def inputs(self, rows):
        return self.joints[rows], self.j2d[rows], self.K[rows], self.weight[rows]


@pytest.fixture(scope='module')
def pool():
    return Pool()


# ---- 1. the per-pose solve ----
@pytest.mark.parametrize('n_iters', pc.GPU_ITERS)
@pytest.mark.parametrize('B', pc.GPU_BATCHES)
def test_translation_against_the_float64_restatement(pool, B, n_iters):
    trans, err_lin, err, status = _run(*pool.inputs(slice(0, B)), n_iters)
    ref = {k: v[:B] for k, v in pool.ref[n_iters].items() if k in ('trans', 'trans_linear', 'err_lin', 'err', 'status')}
    assert trans.dtype == F64 and err.dtype == F and status.dtype == np.int32
    assert np.array_equal(status, ref['status'])
    bad = (ref['status'] & pc.BAD_BITS) != 0
    assert B < 65 or bad.any()
    for got, want in ((trans, ref['trans']), (err_lin, ref['err_lin']), (err, ref['err'])):
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all()
    d_t = np.abs(trans - ref['trans'])[~bad].max()
    d_l, d_e = np.abs(err_lin.astype(F64) - ref['err_lin'])[~bad].max(), np.abs(err.astype(F64) - ref['err'])[~bad].max()
    same = np.array_equal(_bits(trans[~bad]), _bits(ref['trans'][~bad]))
    print(f'B {B} steps {n_iters}: trans {d_t:.3e} m (bound 1e-7; bits equal: {same}), err_lin {d_l:.3e} px, err {d_e:.3e} px (bound 1e-3)')
    assert d_t <= 1e-7 and d_l <= 1e-3 and d_e <= 1e-3
    if n_iters == 0:                                                                   # no step: the linear start is the result
        assert np.array_equal(_bits(err), _bits(err_lin))
        assert np.abs(trans - ref['trans_linear'])[~bad].max() <= 1e-7
    if n_iters == 10:                                                                  # the same bits alone and inside the 1000
        for got, whole in zip((trans, err_lin, err, status), pool.whole):
            assert np.array_equal(_bits(got), _bits(whole[:B]))


def test_exact_pixels_recover_the_planted_translation_and_noise_is_refined(pool):
    trans, err_lin, err, status = pool.whole
    exact = pool.regular & (np.arange(pc.GPU_POOL) % 2 == 0)
    d = np.abs(trans - pool.planted)[exact].max()
    print(f'planted translation recovered to {d:.3e} m on {exact.sum()} exact poses; mean error of the noisy ones '
          f'{err_lin[pool.regular & ~exact].mean():.4f} -> {err[pool.regular & ~exact].mean():.4f} px')
    assert d <= 1e-5
    part = pool.weight > 0
    noisy = pool.regular & ~exact
    cost = lambda e: (pool.weight * e.astype(F64) ** 2 * part).sum(1)
    assert (cost(err)[noisy] <= cost(err_lin)[noisy] * (1 + 1e-6)).all() and (cost(err)[noisy] < cost(err_lin)[noisy]).mean() > 0.9


def test_a_pose_keeps_its_bits_alone_at_another_place_and_in_a_second_call(pool):
    again = _run(pool.joints, pool.j2d, pool.K, pool.weight, 10)
    for a, b in zip(again, pool.whole):
        assert np.array_equal(_bits(a), _bits(b))
    for i in (0, 70, 256, 999):                                                        # alone, and inside a batch of 257 at another lane
        alone = _run(*pool.inputs(slice(i, i + 1)), 10)
        rows = np.concatenate([np.arange(300, 300 + 130), [i], np.arange(450, 450 + 126)])
        inside = _run(*pool.inputs(rows), 10)
        for a, b, w in zip(alone, inside, pool.whole):
            assert np.array_equal(_bits(a[0]), _bits(w[i])) and np.array_equal(_bits(b[130]), _bits(w[i]))


def test_null_weights_are_ones_and_err_lin_is_optional(pool):
    rows = slice(0, 130)
    j, p, K, _ = pool.inputs(rows)
    ones = _run(j, p, K, np.ones((130, 17), F), 10)
    none = _run(j, p, K, None, 10)
    for a, b in zip(ones, none):
        assert np.array_equal(_bits(a), _bits(b))
    short = _run(j, p, K, None, 10, want_linear=False)
    assert np.array_equal(_bits(short[0]), _bits(none[0])) and np.array_equal(_bits(short[2]), _bits(none[2]))
    # a weight-zero joint does not move the result, whatever stands in it
    w = pool.weight[rows].copy()
    base = _run(j, p, K, w, 10)
    j2, p2 = j.copy(), p.copy()
    dropped = w == 0
    assert dropped.any()
    j2[dropped] += F(0.3)
    p2[dropped] -= F(200.0)
    moved = _run(j2, p2, K, w, 10)
    assert np.array_equal(_bits(moved[0]), _bits(base[0])) and np.array_equal(moved[3], base[3])
    assert np.array_equal(_bits(moved[2][~dropped]), _bits(base[2][~dropped]))


# ---- 2. the projection ----
@pytest.mark.parametrize('N', pc.PROJECT_POINTS)
def test_project_points_against_float64(N):
    eng = _mod('engine')
    points, trans, K = pc.project_case(N)
    B = points.shape[0]
    uv_f, d_f = torch.full((B + 2, N, 2), SENTINEL, device=DEV), torch.full((B + 2, N), SENTINEL, device=DEV)
    eng.project_points(_dev(points), _dev(trans), _dev(K), out=(uv_f[1:B + 1], d_f[1:B + 1]))
    uv_h, d_h = uv_f.cpu().numpy(), d_f.cpu().numpy()
    assert (uv_h[[0, B + 1]] == SENTINEL).all() and (d_h[[0, B + 1]] == SENTINEL).all()
    uv, depth = uv_h[1:B + 1], d_h[1:B + 1]
    want, want_d, bound = pc.project_reference(points, trans, K)
    behind = np.isnan(want[..., 0])
    assert behind.any() and not behind.all() and behind[1, 0]                            # the case set holds points with Z <= 0
    assert np.array_equal(np.isnan(uv), np.isnan(want))
    ratio = np.nanmax(np.abs(uv.astype(F64) - want) / bound)
    print(f'N {N}: largest |difference| / bound {ratio:.3f}; {behind.sum()} of {behind.size} points not in front')
    assert ratio <= 1.0
    assert np.abs(depth.astype(F64) - want_d).max() <= 2.0 ** -23 * np.abs(want_d).max() + 1e-9 and (N == 1 or depth[1, 0] == 0.0)
    # without the depth output, and through the plain return value
    plain = eng.project_points(_dev(points), _dev(trans), _dev(K))
    assert np.array_equal(_bits(plain.cpu().numpy()), _bits(uv))


def test_projection_of_the_placed_joints_is_the_error_the_solve_reports(pool):
    rows = np.nonzero(pool.regular)[0][:200]
    j, p, K, _ = pool.inputs(rows)
    trans, err = pool.whole[0][rows], pool.whole[2][rows]
    uv = _mod('engine').project_points(_dev(j), _dev(trans), _dev(K)).cpu().numpy()
    d = np.linalg.norm(uv.astype(F64) - p, axis=-1)
    assert np.abs(d - err).max() <= 2e-3                                               # fp32 pixels of ~1e3: 2^-13 px per coordinate


# ---- 3. the table ----
def _table(trans, err_lin, err, weight, status, group, n_groups, acc=None):
    words = n_groups * pc.ROW + pc.TRAILER
    frame = torch.full((words + 16,), -99, dtype=torch.int64, device=DEV)
    frame[8:8 + words] = 0 if acc is None else T(acc).to(DEV)
    _mod('engine').place_accumulate(_dev(trans), _dev(err_lin), _dev(err), _dev(weight), _dev(status), _dev(group), n_groups, frame[8:8 + words])
    host = frame.cpu().numpy()
    assert (host[:8] == -99).all() and (host[8 + words:] == -99).all()
    return host[8:8 + words].copy()


def test_table_is_exactly_the_integer_accumulation_of_what_the_kernel_wrote(pool):
    trans, err_lin, err, status = pool.whole
    n = 330
    group = (np.arange(n) % 4).astype(np.int32)
    group[[5, 77]], group[130] = -1, 4                                                 # two ignored, one outside the table
    args = (trans[:n], err_lin[:n], err[:n], pool.weight[:n], status[:n], group)
    table = _table(*args, 4)
    want = pc.accumulate(*args, 4)
    assert table.dtype == np.int64 and np.array_equal(table, want)
    rows = table[:-2].reshape(4, pc.ROW)
    assert table[-2:].tolist() == [2, 1] and int(rows[:, pc.BAD].sum()) == 4 and int(rows[:, pc.COUNT].sum()) == n - 3 - 4
    assert (rows[:, pc.JOINTS:pc.JOINTS + 17] <= rows[:, [pc.COUNT]]).all() and (rows[:, pc.JOINTS:pc.JOINTS + 17] < rows[:, [pc.COUNT]]).any()
    # two shards summed equal one call, in either form; a permutation gives the same table
    first = _table(*(a[:100] for a in args), 4)
    assert first.any() and np.array_equal(_table(*(a[100:] for a in args), 4, acc=first), table)
    assert np.array_equal(first + _table(*(a[100:] for a in args), 4), table)
    perm = np.random.RandomState(1).permutation(n)
    assert np.array_equal(_table(*(a[perm] for a in args), 4), table)
    # no groups, no weights, no linear errors
    bare = _table(trans[:n], None, err[:n], None, status[:n], None, 1)
    assert np.array_equal(bare, pc.accumulate(trans[:n], None, err[:n], None, status[:n], None, 1))
    assert not bare[pc.SUM_ERR_LIN:pc.SUM_ERR_LIN + 17].any() and (bare[pc.JOINTS:pc.JOINTS + 17] == bare[pc.COUNT]).all() and bare[-2:].tolist() == [0, 0]
    # a status bit 3 and an absurd value: counted in their words only
    st = status[:70].copy()
    st[[3, 66]] |= pc.BIT_STEP
    e = err[:70].copy()
    e[10, 2] = 2000.0
    t3 = _table(trans[:70], err_lin[:70], e, None, st, None, 1)
    assert np.array_equal(t3, pc.accumulate(trans[:70], err_lin[:70], e, None, st, None, 1)) and t3[pc.STEP_PIVOT] == 2 and t3[pc.BAD] == 3 + 1      # the refusals at 1, 40 and 64, and pose 10
    doc = _mod('place_report').derive(table_ok := _table(*args[:5], np.where(group == 4, 3, group), 4), list('abcd'))
    assert table_ok[-1] == 0 and doc['all']['n'] == n - 2 - 4 and doc['all']['n_bad'] == 4
    good = (status[:n] == 0) & (group >= 0)
    np.testing.assert_allclose(doc['all']['depth_m'], trans[:n][good, 2].mean(), rtol=1e-6)
    with pytest.raises(RuntimeError, match='1 poses carried a group id outside'):
        _mod('place_report').derive(table, list('abcd'))


# ---- 4. the refusals ----
def test_every_refusal_returns_non_zero_with_its_message_and_touches_nothing(pool):
    lm = _mod('_lib')
    lib, ptr, sp = lm.load(), lm.ptr, lm.stream_ptr(torch.device(DEV))
    B = 70
    j, p, K, w = (_dev(a) for a in pool.inputs(slice(0, B)))
    trans = torch.full((B + 1, 3), SENTINEL, dtype=torch.float64, device=DEV)
    err_lin, err = torch.full((B, 17), SENTINEL, device=DEV), torch.full((B, 17), SENTINEL, device=DEV)
    status = torch.full((B,), -99, dtype=torch.int32, device=DEV)
    uv, acc = torch.full((B, 17, 2), SENTINEL, device=DEV), torch.full((2 * pc.ROW + 2,), -99, dtype=torch.int64, device=DEV)
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)

    def place(joints=ptr(j), j2d=ptr(p), Km=ptr(K), weight=ptr(w), batch=B, n_iters=10, tr=ptr(trans), el=ptr(err_lin), e=ptr(err), st=ptr(status)):
        return lib.jrr_place_translation(joints, j2d, Km, weight, batch, n_iters, tr, el, e, st, sp)

    def project(points=ptr(j), tr=ptr(trans), Km=ptr(K), batch=B, n=17, out=ptr(uv), depth=None):
        return lib.jrr_project_points(points, tr, Km, batch, n, out, depth, sp)

    def accumulate(tr=ptr(trans), el=ptr(err_lin), e=ptr(err), weight=None, st=ptr(status), group=None, batch=B, n_groups=2, table=ptr(acc)):
        return lib.jrr_place_accumulate(tr, el, e, weight, st, group, batch, n_groups, table, sp)

    refusals = [(place, dict(joints=None), 'jrr_place_translation: bad argument'), (place, dict(j2d=None), 'bad argument'),
                (place, dict(Km=None), 'bad argument'), (place, dict(tr=None), 'jrr_place_translation: no output'),
                (place, dict(e=None), 'no output'), (place, dict(st=None), 'no output'),
                (place, dict(batch=-1), 'jrr_place_translation: batch must not be negative'),
                (place, dict(n_iters=-1), 'jrr_place_translation: n_iters -1: 0 .. 64'), (place, dict(n_iters=65), 'n_iters 65: 0 .. 64'),
                (place, dict(tr=off(trans, 4)), 'jrr_place_translation: trans must be 8-byte aligned'),
                (place, dict(joints=off(j, 2)), '4-byte aligned'),
                (project, dict(points=None), 'jrr_project_points: bad argument'), (project, dict(tr=None), 'bad argument'),
                (project, dict(Km=None), 'bad argument'), (project, dict(out=None), 'jrr_project_points: no output'),
                (project, dict(batch=-1), 'jrr_project_points: batch must not be negative'),
                (project, dict(n=-1), 'jrr_project_points: n_points must not be negative'),
                (project, dict(batch=1 << 20, n=1 << 11), 'jrr_project_points: batch * n_points must stay below 2^31'),
                (project, dict(tr=off(trans, 4)), 'jrr_project_points: trans must be 8-byte aligned'),
                (accumulate, dict(tr=None), 'jrr_place_accumulate: bad argument'), (accumulate, dict(e=None), 'bad argument'),
                (accumulate, dict(st=None), 'bad argument'), (accumulate, dict(table=None), 'bad argument'),
                (accumulate, dict(batch=-1), 'jrr_place_accumulate: batch must not be negative'),
                (accumulate, dict(n_groups=0), 'jrr_place_accumulate: n_groups 0: 1 .. 1024'), (accumulate, dict(n_groups=1025), 'n_groups 1025: 1 .. 1024'),
                (accumulate, dict(table=off(acc, 4)), 'jrr_place_accumulate: trans and acc must be 8-byte aligned'),
                (accumulate, dict(tr=off(trans, 4)), 'trans and acc must be 8-byte aligned')]
    for fn, kw, message in refusals:
        rc = fn(**kw)
        assert rc != 0 and message in lib.jrr_last_error().decode(), (kw, rc, lib.jrr_last_error())
    torch.cuda.synchronize()
    assert (trans == SENTINEL).all().item() and (err_lin == SENTINEL).all().item() and (err == SENTINEL).all().item()
    assert (status == -99).all().item() and (uv == SENTINEL).all().item() and (acc == -99).all().item()
    # batch 0 (and no points): a clean no-op
    assert place(batch=0) == 0 and project(batch=0) == 0 and project(n=0) == 0 and accumulate(batch=0) == 0
    torch.cuda.synchronize()
    assert (trans == SENTINEL).all().item() and (status == -99).all().item() and (uv == SENTINEL).all().item() and (acc == -99).all().item()
    eng = _mod('engine')
    empty = eng.place_translation(j[:0], p[:0], K[:0], None, 10)
    assert empty[0].shape == (0, 3) and empty[3].shape == (0,)
    with pytest.raises(ValueError, match='n_iters 65'):
        eng.place_translation(j, p, K, None, 65)


# ---- 5. the command ----
def _with_args(flags, fn):
    argsmod = _mod('args')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(flags + ['--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent'])
    try:
        torch.manual_seed(0)
        return fn()
    finally:
        argsmod._LazyArgs._ns = saved


def _write_split(root, tensors, paths):
    d = os.path.join(root, 'precomputed_val')
    os.makedirs(d, exist_ok=True)
    for k, v in tensors.items():
        torch.save(v, os.path.join(d, f'{k}.pt'))
    with open(os.path.join(d, 'images.pkl'), 'wb') as f:
        pickle.dump(paths, f)


def test_the_place_refined_command_end_to_end(tmp_path, smpl_model_np, j_h36m_np):
    """a 12-sample split: the driver writes a table from it, gt_j2d is then made by projecting the table's OWN joints with planted
    translations under per-sample intrinsics, and the command recovers them"""
    n = 12
    sm, refined, eng, utils = _mod('smpl_model'), _mod('refined'), _mod('engine'), _mod('utils')
    root = str(tmp_path / 'data')
    full = sm.synthetic_batch(smpl_model_np, j_h36m_np, n, seed=0)
    rng = np.random.RandomState(3)
    aa = rng.normal(0, 0.3, size=(n, 24, 3)).astype(F)
    paths = [f'/data/h36m/S9/{"Walking 1" if i < 7 else "Eating"}/imageSequence/1/img_{i + 1:06d}.jpg' for i in range(n)]
    K = pc.cameras(n, rng)
    tensors = {'bboxes': torch.tensor([[100., 200., 700., 800.]]).repeat(n, 1), 'betas': T(full['betas']), 'estimated_translation': T(full['cam']),
               'gt_j2d': torch.rand(n, 17, 2) * 1000, 'gt_j3d': T(full['gt_j3d']), 'intrinsics': T(K), 'orient': T(aa[:, 0]),
               'pose': T(aa[:, 1:].reshape(n, 69))}
    _write_split(root, tensors, paths)
    out_dir = os.path.join(root, 'refined')
    flags = ['--batch_size', '8', '--inner_iters', '2', '--device', DEV, '--synthetic', '--data_root', root]
    _with_args(flags + ['--save_refined', out_dir], lambda: _mod('optimize').optimize_pose_refiner(log=lambda r: None))
    raw = refined.load(out_dir, n=n)
    assert raw['has_refined'].all()
    # the table's own joints: the initial regressor, the driver's body
    smpl = importlib.import_module(f'{PKG_NAME}.smpl').SMPL('/nonexistent', batch_size=1, allow_synthetic=True).to(torch.device(DEV))
    J = T(sm.default_h36m_regressor('/nonexistent', allow_default=True)).float().to(DEV)
    e = eng.RefineEngine(smpl.device_model, n)
    e.set_j_regressor(J, utils.find_j_reg_mask(J))
    joints = e.find_joints_forward(T(raw['shape']).to(DEV), x6d=T(raw['pose6d']).to(DEV)).float().cpu().numpy()
    planted = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2.5, 7.0, n)], 1)
    tensors['gt_j2d'] = T(pc.project64(joints, planted, K)[0].astype(F))
    _write_split(root, tensors, paths)
    raw_bytes = open(os.path.join(out_dir, 'refined.npz'), 'rb').read()
    lines = []
    out = _with_args(['--place_refined', out_dir, '--data_root', root, '--synthetic', '--device', DEV, '--batch_size', '8'],
                     lambda: refined.place_command(log=lines.append))
    assert sorted(os.listdir(out_dir)) == ['meta.json', 'place.json', 'place.md', 'refined.npz', 'refined_placed.npz']
    assert open(os.path.join(out_dir, 'refined.npz'), 'rb').read() == raw_bytes           # the input keeps its bytes
    back = refined.load(out_dir, n=n, name=refined.PLACE_NAME)
    d = np.abs(back['trans'] - planted).max()
    print(lines[0])
    print(f'planted translations recovered to {d:.3e} m (bound 1e-5); reprojection {back["reproj_px"].max():.3e} px')
    assert d <= 1e-5 and back['trans'].dtype == F64 and back['trans_linear'].dtype == F64 and (back['place_status'] == 0).all()
    assert back['reproj_px'].shape == (n, 17) and back['reproj_px'].dtype == F and back['reproj_px'].max() < 1e-2
    assert np.abs(back['trans_linear'] - planted).max() <= 1e-5 and back['reproj_px_linear'].dtype == F
    for k in raw:
        if k != 'meta':
            assert np.array_equal(back[k], raw[k], equal_nan=True), k
    assert all(np.array_equal(back[k], out[k], equal_nan=True) for k in back if k != 'meta')
    doc = _mod('place_report').load(out_dir)
    assert doc['groups'] == ['Eating', 'Walking'] and doc['n_iters'] == 10 and doc['table']['all']['n'] == n and doc['table']['groups']['Walking']['n'] == 7
    assert 'root_err_mm' not in doc['table']['all']                                     # this split's gt_j3d is pelvis-centred
    np.testing.assert_allclose(doc['table']['all']['depth_m'], planted[:, 2].mean(), rtol=1e-6)
    assert len(lines) == 1 and lines[0].startswith(f'placed {n} poses (10 steps')
    meta = json.load(open(os.path.join(out_dir, 'meta.json')))
    assert meta['place']['placed'] == n and meta['place']['n_iters'] == 10 and {k: v for k, v in meta.items() if k != 'place'} == raw['meta']
    # the placed file feeds a run as the smoothed one does
    again = _with_args(flags[:2] + ['--inner_iters', '0'] + flags[4:] + ['--init_refined', os.path.join(out_dir, refined.PLACE_NAME)],
                       lambda: _mod('optimize').optimize_pose_refiner(log=lambda r: None))
    idx = again['index'].numpy()
    assert np.array_equal(again['x6d'].cpu().numpy(), back['pose6d'][idx]) and np.array_equal(again['betas'].cpu().numpy(), back['shape'][idx])
