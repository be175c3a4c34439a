"""The exact solve of the regressor fit on the GPU (pytest -m gpu): jrr_jfit_moments against numpy (int64 on integer inputs, float64
otherwise), jrr_jfit_set_entries against the float64 restatement of tests/jfit_cases.py, the solve's certificate against Adam, the
argument checks, and the `--fit_solve` command as a child process.

Bounds.  Integer inputs (vertices in [-512, 512], ground truth in [-1000, 1000] mm, as fp32): every product and every sum is an
integer below 2^53, so M equals numpy's int64 result element for element -- the layout test.  Real inputs: a sum of exactly formed
products, |M - M_f64| <= 3 count 2^-53 sum|a||b| elementwise (M_f64: the definition's sums rounded to float64 -- taken in extended
precision, jsolve_cases.moments_reference, so that the reference's own float64 rounding, which may reach the same size, does not
use up the kernel's bound; the distance from numpy's plain float64 sums is printed beside it).  The loss from the moments against
jrr_jfit_run's own loss: rtol 1e-5.  The forward after set_entries: jfit_cases.bound of the restatement's
float32 and float64 evaluations.

Shapes: ns = 4, 21, 62, 83 (W = ns + 17 = 21, 38, 79, 100: no multiple of 16; 2 x 2, 3 x 3, 5 x 5 and 7 x 7 tiles, i.e. 3, 6, 15 and
28 upper-triangular tiles: below, at and above the 16 tiles of one workgroup); counts 1, 3, 149 from row 7 (three row chunks), 1500
(24 row chunks of 63 and 51: JRR_JFIT_MOM_CHUNK = 64 rows per chunk at most; six slabs per group of the second launch) and 2200 (35
chunks: the four groups of the second launch add 9, 9, 9 and 8 slabs, eight loads in flight and one behind them)."""
import ctypes
import importlib
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import jfit_cases as fc
import jsolve_cases as jc
from conftest import PKG_NAME, ROOT

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
NS = (4, 21, 62, 83)
RANGES = ((0, 1), (5, 3), (7, 149), (3, 1500), (9, 2200), (2209, 1), (0, 0))
N_ROWS = 2210


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _fit(J, rows):
    """a RegressorFit of J whose cache rows are `rows` (n, ns + 17, 3), written directly"""
    fit = _mod('engine').RegressorFit(T(J).to(DEV), None, len(rows))
    W = fit.ns + 17
    assert rows.shape[1:] == (W, 3)
    fit.cache[:, :3 * W] = T(np.ascontiguousarray(rows.reshape(len(rows), 3 * W))).to(DEV)
    return fit


# ---- 1. the moments ----
@pytest.mark.parametrize('ns', NS)
def test_moments_of_integers_are_exact(ns):
    J, cols = jc.regressor_with_union(ns)
    rows = jc.integer_rows(ns, N_ROWS, ns)
    fit = _fit(J, rows)
    assert fit.ns == ns
    for begin, count in RANGES:
        got = fit.moments(begin, count).cpu().numpy()
        want = jc.moments(rows[begin:begin + count], np.int64)
        assert got.shape == (ns + 17, ns + 17) and got.dtype == np.float64
        assert np.abs(want).max() < 2 ** 53 if count else not got.any()
        wrong = int((got != want.astype(np.float64)).sum())
        print(f'ns {ns} rows [{begin}, {begin + count}): {wrong} of {got.size} elements differ')
        assert wrong == 0
    fit.info()


@pytest.mark.parametrize('ns', NS)
def test_moments_of_real_inputs(ns):
    J, cols = jc.regressor_with_union(ns)
    rows = jc.real_rows(ns, N_ROWS, ns)
    fit = _fit(J, rows)
    for begin, count in RANGES[:-1]:
        got = fit.moments(begin, count).cpu().numpy()
        again = fit.moments(begin, count).cpu().numpy()
        want, mag = jc.moments_reference(rows[begin:begin + count]), jc.abs_moments(rows[begin:begin + count])
        bound = 3.0 * count * 2.0 ** -53 * mag
        plain = jc.moments(rows[begin:begin + count])
        on = bound > 0                                              # (the pelvis of the ground truth is the origin: zero rows and columns)
        print(f'ns {ns} rows [{begin}, {begin + count}): worst {np.max(np.abs(got - want)[on] / bound[on]):.3f} of the bound '
              f'({np.max(np.abs(got - plain)[on] / bound[on]):.3f} against numpy\'s own float64 sums)')
        assert (np.abs(got - want) <= bound).all()
        assert np.array_equal(got.view(np.uint64), got.T.copy().view(np.uint64))
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64))


@pytest.mark.parametrize('ns', [21, 83])
def test_loss_from_moments_is_the_step_kernels_loss(ns):
    rs = _mod('regressor_solve')
    J, cols = jc.regressor_with_union(ns)
    rows = jc.real_rows(ns + 1, 298, ns)
    fit = _fit(J, rows)
    M = fit.moments(149, 149).cpu().numpy()
    want = float(fit.run(149, 1, 1, 1e-2).cpu().numpy()[0])          # the loss BEFORE the update: J_init's
    got, _ = rs.loss_from_moments(M, 149, jc.lists_of(J, cols), jc.normalised_rows(J, cols))
    print(f'ns {ns}: loss {got:.9e} from the moments, {want:.9e} from jrr_jfit_run')
    assert abs(got - want) <= 1e-5 * abs(want)


# ---- 2. set_entries ----
@pytest.fixture(scope='module')
def case():
    return fc.trajectory_case()


def _gathered(c):
    fit = _mod('engine').RegressorFit(T(c['J']).to(DEV), T(c['mask']).to(DEV), len(c['verts']))
    fit.gather(T(c['verts']).to(DEV), T(c['gt']).to(DEV), 0)
    return fit


def test_set_entries(case):
    c = case
    fit = _gathered(c)
    fit.run(fc.BATCH, 0, 3, fc.LR)
    assert fit.info()[2] == 3
    rng = np.random.RandomState(3)
    listed = np.zeros(c['J'].shape, dtype=bool)
    for i, v in enumerate(c['vtx']):
        listed[i, v] = True
    J2 = rng.uniform(-1, 1, size=c['J'].shape).astype(np.float32)   # elements outside the lists are not read
    J2[listed] = rng.uniform(0.0, 1.0, size=int(listed.sum())).astype(np.float32)
    J2[1, c['vtx'][1][::3]] = 0.0                                  # zeros and a negative value among the listed entries
    J2[16, c['vtx'][16][5]] = -0.25
    fit.set_entries(T(J2).to(DEV))
    assert fit.info() == (211, 260, 0, list(fc.COUNTS))            # the step counter reads 0
    want = np.where(listed, J2, c['J'])
    got = fit.joints().cpu().numpy()
    j64 = fc.Restatement(want, c['mask'], dtype=fc.F64).joints(c['verts'])
    j32 = fc.Restatement(want, c['mask'], dtype=fc.F32).joints(c['verts'])
    b = fc.bound(j32, j64)
    print(f'joints after set_entries: {fc.dist(got, j64):.3e} from float64 (bound {b:.3e})')
    assert fc.dist(got, j64) <= b
    Jd, m, v = (t.cpu().numpy() for t in fit.dense())
    assert np.array_equal(Jd.view(np.uint32), want.view(np.uint32)) and not m.any() and not v.any()
    # Adam starts again from step 0: one step equals the first step of a restatement that starts at these values
    grad = torch.zeros(17, 128, device=DEV)
    fit.run(fc.BATCH, 0, 1, fc.LR, grad=grad)
    r32, r64 = fc.Restatement(want, c['mask'], dtype=fc.F32), fc.Restatement(want, c['mask'], dtype=fc.F64)
    for r in (r32, r64):
        r.step(c['verts'][:fc.BATCH], c['gt'][:fc.BATCH])
    assert fc.dist(fit.dense()[0].cpu().numpy(), r64.raw()) <= fc.bound(r32.raw(), r64.raw()) and fit.info()[2] == 1
    assert not (fit.dense()[0].cpu().numpy()[1, c['vtx'][1][::3]] != 0).any()        # a listed entry at zero does not move
    # a row set to all zeros is reported by info(), until a later set_entries repairs it
    J3 = want.copy()
    J3[4, c['vtx'][4]] = 0.0
    fit.set_entries(T(J3).to(DEV))
    with pytest.raises(_mod('_lib').JrrError, match='without a positive entry'):
        fit.info()
    fit.set_entries(T(want).to(DEV))
    assert fit.info()[2] == 0


def test_a_state_prepared_from_a_candidate_pattern(case):
    """--fit_rings: the state is prepared from ones on the candidates and given the true initial values with set_entries; the zero
    entries add nothing to the forward, so the joints are the bits of a state prepared from the values themselves"""
    c = case
    J, vtx = c['J'] * c['mask'], c['vtx']
    pattern = (J > 0).astype(np.float32)
    for i in (0, 2, 5):                                             # further candidates inside the union of the other rows: NS stays 211
        pool = np.setdiff1d(np.unique(np.concatenate(vtx)), vtx[i])
        pattern[i, pool[:7]] = 1.0
    em = _mod('engine')
    fit = em.RegressorFit(T(pattern).to(DEV), None, len(c['verts']))
    assert fit.ns == 211 and fit.entries == 260 + 21
    fit.J_init = T(J.astype(np.float32)).to(DEV)
    fit.gather(T(c['verts']).to(DEV), T(c['gt']).to(DEV), 0)
    fit.set_entries(fit.J_init)
    plain = em.RegressorFit(T(J.astype(np.float32)).to(DEV), None, len(c['verts']))
    plain.gather(T(c['verts']).to(DEV), T(c['gt']).to(DEV), 0)
    # (a row's sum and a step's dot products run over the lanes in list order, which the further candidates shift: last bits may differ)
    assert fc.dist(fit.joints().cpu().numpy(), plain.joints().cpu().numpy()) <= 1e-6 and torch.equal(fit.dense()[0], plain.dense()[0])
    assert torch.equal(fit.moments(), plain.moments())
    la, lb = fit.run(fc.BATCH, 0, 3, fc.LR).cpu().numpy(), plain.run(fc.BATCH, 0, 3, fc.LR).cpu().numpy()
    assert la[0] == pytest.approx(lb[0], rel=1e-6) and np.allclose(la[:3], lb[:3], rtol=1e-5, atol=0)
    Ja, Jb = fit.dense()[0].cpu().numpy(), plain.dense()[0].cpu().numpy()
    extra = (pattern > 0) & ~(J > 0)
    assert np.array_equal(Ja[extra], J[extra].astype(np.float32)) and int(extra.sum()) == 21      # Adam cannot move the zero candidates
    assert fc.dist(Ja, Jb) <= 1e-5 and (Ja != J.astype(np.float32))[J > 0].all()


# ---- 3. Adam against the certificate ----
def _device_case(name, rings):
    """a jsolve case as a regressor on 6890 columns and its cache rows: the union is the vertices the lists use"""
    c = jc.table(name)
    lists = c['lists1'] if rings else c['lists0']
    x0 = c['x0_1'] if rings else c['x0']
    used = np.unique(np.concatenate(lists))
    cols = np.sort(np.random.RandomState(5).choice(fc.V, used.size, replace=False))
    J = np.zeros((17, fc.V), dtype=np.float32)
    for i, l in enumerate(lists):
        J[i, cols[np.searchsorted(used, l)]] = x0[i].astype(np.float32)
    rows = jc.rows_of(c['points'][:, used], c['gt'])
    return J, cols, [np.searchsorted(used, l) for l in lists], rows


def test_adam_approaches_the_certificate_and_never_passes_it():
    rs = _mod('regressor_solve')
    J, cols, lists, rows = _device_case('body', 0)
    n = len(rows)
    fit = _fit(J, rows)
    assert [l.size for l in lists] == fit.counts
    M = fit.moments(0, n).cpu().numpy()
    x0 = [J[i, cols[l]].astype(np.float64) for i, l in enumerate(lists)]
    r = rs.solve(M, n, lists, x0, tol=jc.TOL, max_iter=jc.MAX_ITER)
    assert r['converged'] and r['gap'] <= jc.TOL * r['loss0']
    losses = fit.run(n, 0, 1, fc.LR).cpu().numpy()[:1].astype(np.float64)
    for _ in range(29):
        losses = np.append(losses, fit.run(n, 0, 1, fc.LR).cpu().numpy()[0])
    floor = r['loss'] - r['gap'] - 1e-5 * r['loss']
    print(f'solve: {r["loss0"]:.6e} -> {r["loss"]:.6e} (gap {r["gap"]:.2e}, {r["iterations"]} steps); Adam: {losses[0]:.6e} -> '
          f'{losses.min():.6e} over 30 steps')
    assert abs(losses[0] - r['loss0']) <= 1e-5 * r['loss0']
    assert (losses >= floor).all() and losses[-1] < losses[0]
    # the solved weights through set_entries: the step kernel's loss there is the solve's
    Jx = J.copy()
    for i, l in enumerate(lists):
        Jx[i, cols[l]] = r['x'][i].astype(np.float32)
    fit.set_entries(T(Jx).to(DEV))
    at = float(fit.run(n, 0, 1, fc.LR).cpu().numpy()[0])
    print(f'the step kernel at the solved weights: {at:.9e} against {r["loss"]:.9e}')
    assert abs(at - r['loss']) <= 2e-5 * r['loss']                 # 1e-5 for the kernel's loss, as much again for weights rounded to fp32
    fit.info()


# ---- 4. argument checks ----
def test_argument_checks():
    lib_mod = _mod('_lib')
    lib = lib_mod.load()
    J, cols = jc.regressor_with_union(21)
    rows = jc.real_rows(1, 150, 21)
    fit = _fit(J, rows)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    need = ctypes.c_size_t(0)
    assert lib.jrr_jfit_moments_bytes(21, ctypes.byref(need)) == 38 * 38 * 8 and need.value >= 6 * 256 * 8
    assert lib.jrr_jfit_moments_bytes(21, None) == 38 * 38 * 8
    assert lib.jrr_jfit_moments_bytes(0, ctypes.byref(need)) == 0 and need.value == 0 and lib.jrr_jfit_moments_bytes(2177, None) == 0
    lib.jrr_jfit_moments_bytes(21, ctypes.byref(need))
    M = torch.zeros(38, 38, dtype=torch.float64, device=DEV)
    scratch = torch.zeros(need.value // 8, dtype=torch.float64, device=DEV)
    sb = need.value
    state0 = fit.state.clone()
    call = lambda st, ca, n_rows, begin, count, ns, m, sc, nbytes: lib.jrr_jfit_moments(st, ca, n_rows, begin, count, ns, m, sc, nbytes, None)
    assert call(P(fit.state), P(fit.cache), 150, 0, 150, 21, P(M), P(scratch), sb) == 0
    bad = [
        call(None, P(fit.cache), 150, 0, 150, 21, P(M), P(scratch), sb),
        call(P(fit.state), None, 150, 0, 150, 21, P(M), P(scratch), sb),
        call(P(fit.state), P(fit.cache), 150, 0, 150, 21, None, P(scratch), sb),
        call(P(fit.state), P(fit.cache), 150, 0, 150, 21, P(M), None, sb),
        call(P(fit.state), P(fit.cache), 150, -1, 10, 21, P(M), P(scratch), sb),
        call(P(fit.state), P(fit.cache), 150, 0, 151, 21, P(M), P(scratch), sb),
        call(P(fit.state), P(fit.cache), 150, 100, 51, 21, P(M), P(scratch), sb),
        call(P(fit.state), P(fit.cache), 150, 151, 0, 21, P(M), P(scratch), sb),
        call(P(fit.state), P(fit.cache), 150, 0, -1, 21, P(M), P(scratch), sb),
        call(P(fit.state), P(fit.cache), -1, 0, 0, 21, P(M), P(scratch), sb),
        call(P(fit.state), P(fit.cache), 150, 0, 150, 0, P(M), P(scratch), sb),
        call(P(fit.state), P(fit.cache), 150, 0, 150, 17 * 128 + 1, P(M), P(scratch), sb),
        call(P(fit.state), ctypes.c_void_p(fit.cache.data_ptr() + 4), 150, 0, 150, 21, P(M), P(scratch), sb),
        call(P(fit.state), P(fit.cache), 150, 0, 150, 21, ctypes.c_void_p(M.data_ptr() + 4), P(scratch), sb),
        lib.jrr_jfit_set_entries(None, P(fit.J_init), None),
        lib.jrr_jfit_set_entries(P(fit.state), None, None),
    ]
    assert bad == [-1] * len(bad), bad
    assert b'jrr_jfit_set_entries' in lib.jrr_last_error()
    assert call(P(fit.state), P(fit.cache), 150, 0, 150, 21, P(M), P(scratch), sb - 8) == -3          # a short scratch
    assert b'jrr_jfit_moments_bytes' in lib.jrr_last_error()
    torch.cuda.synchronize()
    assert torch.equal(fit.state, state0)                           # no refused call touched the state
    fit.info()
    # a foreign ns is found on the device: M is NaN, the error word is set, nothing else is written
    lib.jrr_jfit_moments_bytes(20, ctypes.byref(need))
    M20 = torch.zeros(37, 37, dtype=torch.float64, device=DEV)
    scratch20 = torch.zeros(need.value // 8, dtype=torch.float64, device=DEV)
    assert call(P(fit.state), P(fit.cache), 150, 0, 150, 20, P(M20), P(scratch20), need.value) == 0
    assert torch.isnan(M20).all() and not scratch20.any()
    with pytest.raises(lib_mod.JrrError, match='not the prepared one'):
        fit.info()


# ---- 5. the command ----
N_CMD = 96


def _paths(n):
    """six sequences of 16 frames: two actions x three cameras"""
    return [f'/data/h36m/S9/Act{(i // 16) // 3} 1/imageSequence/{(i // 16) % 3 + 1}/img_{5 * (i % 16 + 1):06d}.jpg' for i in range(n)]


@pytest.fixture(scope='module')
def command_runs(tmp_path_factory, smpl_model_np):
    """a 96-row synthetic --save_refined table with its dataset directory, the same meshes as a vertices directory, the solve from
    either source with --fit_rings 0 and 1, and the evaluation of one checkpoint"""
    em, sm, refined = _mod('engine'), _mod('smpl_model'), _mod('refined')
    root = str(tmp_path_factory.mktemp('solve_data'))
    J_np = sm.default_h36m_regressor('/nonexistent', allow_default=True)
    full = sm.synthetic_batch(smpl_model_np, J_np, N_CMD, seed=5)
    paths, n = _paths(N_CMD), N_CMD
    x6d, betas, cam = (T(full[k]).to(DEV).contiguous() for k in ('pose6d', 'betas', 'cam'))
    eng = em.RefineEngine(em.DeviceModel(smpl_model_np, DEV), n, flags=em.FLAG_KEEP_VERTS)
    eng.set_j_regressor(T(J_np))
    _, verts = eng.find_joints_forward(betas, x6d=x6d, return_verts=True)
    # the ground truth: the joints of ANOTHER regressor on the same support, 2 mm of noise
    rng = np.random.RandomState(11)
    other = np.where(J_np > 0, J_np * rng.uniform(0.3, 3.0, size=J_np.shape), 0)
    other = other / other.sum(1, keepdims=True)
    gt = np.einsum('jv,bvc->bjc', other, verts.cpu().numpy().astype(np.float64)) * 1000.0 + rng.normal(0, 2.0, size=(n, 17, 3))
    gt = gt.astype(np.float32)
    d = os.path.join(root, 'precomputed_val')
    os.makedirs(d)
    tensors = {'bboxes': torch.tensor([[100., 200., 700., 800.]]).repeat(n, 1), 'betas': T(full['betas']),
               'estimated_translation': T(full['cam']), 'gt_j2d': torch.rand(n, 17, 2) * 1000, 'gt_j3d': T(gt),
               'intrinsics': torch.eye(3).repeat(n, 1, 1), 'orient': torch.zeros(n, 3), 'pose': torch.zeros(n, 69)}
    for k, v in tensors.items():
        torch.save(v, os.path.join(d, f'{k}.pt'))
    with open(os.path.join(d, 'images.pkl'), 'wb') as f:
        pickle.dump(paths, f)
    table_dir = os.path.join(root, 'refined')
    table = refined.RefinedTable(n, DEV)
    table.add(torch.arange(n, dtype=torch.int64, device=DEV), x6d, betas, cam)
    table.finish(table_dir, {'data': 'dataset'})
    vdir = os.path.join(root, 'meshes')
    os.makedirs(vdir)
    np.save(os.path.join(vdir, 'vertices.npy'), verts.cpu().numpy())
    np.save(os.path.join(vdir, 'gt_j3d.npy'), gt)
    with open(os.path.join(vdir, 'paths.txt'), 'w') as f:
        f.write('\n'.join(paths) + '\n')
    torch.cuda.synchronize()
    common = ['--synthetic', '--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent', '--device', DEV, '--batch_size', '32']
    outs = {}
    for name, flags in (('table', ['--fit_from', table_dir, '--data_root', root]), ('verts', ['--fit_from', vdir])):
        for rings in (0, 1):
            out = os.path.join(root, f'solve_{name}_{rings}')
            cmd = [sys.executable, os.path.join(ROOT, 'main.py'), '--fit_regressor', out, '--fit_solve', '--fit_rings', str(rings),
                   '--fit_holdout', '0.34'] + flags + common
            r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
            outs[name, rings] = (out, r.stdout)
    rep = os.path.join(root, 'report')
    cmd = [sys.executable, os.path.join(ROOT, 'main.py'), '--eval_vertices', vdir, '--eval_report', rep, '--eval_j_regressor',
           os.path.join(outs['verts', 1][0], 'retrained_J_Regressor.pt')] + common
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return outs, rep, J_np


def _doc(out):
    with open(os.path.join(out, 'solve.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('rings', [0, 1])
@pytest.mark.parametrize('name', ['table', 'verts'])
def test_the_fit_solve_command(command_runs, name, rings):
    outs, rep, J_np = command_runs
    rs, rf, checkpoint = _mod('regressor_solve'), _mod('regressor_fit'), _mod('checkpoint')
    out, stdout = outs[name, rings]
    assert sorted(os.listdir(out)) == ['retrained_J_Regressor.pt', 'solve.json']
    lines = [l for l in stdout.splitlines() if l.startswith('solved the regressor on ')]
    assert len(lines) == 1 and 'gap' in lines[0] and 'converged' in lines[0] and lines[0].endswith('retrained_J_Regressor.pt')
    doc = _doc(out)
    assert sorted(doc) == sorted(rs.SOLVE_KEYS) and doc['layout_version'] == rs.LAYOUT_VERSION
    assert doc['source'] == ('refined' if name == 'table' else 'vertices') and doc['rings'] == rings
    assert doc['rows'] == {'train': 64, 'holdout': 32}
    assert sorted(doc['support']) == sorted(rs.SUPPORT_KEYS) and sorted(doc['loss']) == sorted(rs.LOSS_KEYS)
    print(name, rings, 'loss', doc['loss'], 'gap', doc['gap'], 'steps', doc['iterations'], 'support', sum(doc['support']['before']), '->',
          sum(doc['support']['candidates']), '->', sum(doc['support']['after']), 'MPJPE', doc['initial']['train']['mpjpe_mm'], '->',
          doc['final']['train']['mpjpe_mm'], 'held out', doc['initial']['holdout']['mpjpe_mm'], '->', doc['final']['holdout']['mpjpe_mm'])
    assert doc['converged'] is True and doc['tol'] == 1e-6 and 0.0 <= doc['gap'] <= doc['tol'] * doc['loss']['train_before']
    assert doc['loss']['train_after'] <= doc['loss']['train_before']
    assert doc['final']['train']['mpjpe_mm'] < doc['initial']['train']['mpjpe_mm']
    assert doc['final']['holdout']['mpjpe_mm'] < doc['initial']['holdout']['mpjpe_mm']
    before = [int(c) for c in (J_np > 0).sum(1)]
    assert doc['support']['before'] == before
    assert doc['support']['candidates'] == before if rings == 0 else all(c > b for c, b in zip(doc['support']['candidates'], before))
    assert all(1 <= a <= c for a, c in zip(doc['support']['after'], doc['support']['candidates']))
    for k in ('fit_solve', 'fit_rings', 'fit_solve_tol', 'fit_solve_iters'):
        assert k in doc['flags']
    # the checkpoint: the solved weights are the raw values -- rows on the simplex over the candidates, everything else untouched
    J = checkpoint.load_j_regressor(os.path.join(out, 'retrained_J_Regressor.pt')).numpy()
    assert J.shape == (17, 6890) and doc['support']['after'] == [int(c) for c in (J > 0).sum(1)]
    smpl_faces = _mod('smpl_model').synthetic_smpl(1234)['faces']
    cands = rs.ring_candidates(J_np, smpl_faces, rings)
    assert [v.size for v in cands] == doc['support']['candidates']
    P = rs.candidate_pattern(cands) > 0
    assert np.array_equal(J[~P], J_np[~P]) and (J[P] >= 0).all() and np.allclose(J.sum(1, where=P), 1.0, atol=1e-5)


@pytest.mark.parametrize('name', ['table', 'verts'])
def test_one_ring_cannot_do_worse(command_runs, name):
    outs, rep, J_np = command_runs
    d0, d1 = _doc(outs[name, 0][0]), _doc(outs[name, 1][0])
    assert d1['loss']['train_before'] == pytest.approx(d0['loss']['train_before'], rel=1e-12)
    assert d1['loss']['train_after'] <= d0['loss']['train_after'] + d1['gap']


def test_the_evaluation_accepts_the_solved_checkpoint(command_runs):
    outs, rep, J_np = command_runs
    assert sorted(os.listdir(rep)) == ['eval.json', 'eval.md']
    doc = _mod('eval_report').load(rep)
    assert doc['j_regressor_retrained']['path'].endswith('retrained_J_Regressor.pt')
