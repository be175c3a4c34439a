"""The MPJPE solve of the regressor fit on the GPU (pytest -m gpu): jrr_jfit_norm_moments against jrr_jfit_moments and integer arithmetic
(UNIT mode, the layout), against the restatement of tests/jnorm_cases.py (INV mode), its repeatability and refusals, the MPJPE it
states against jrr_jfit_joints + jrr_evaluate, the solve driven by device passes, and the `--fit_solve_loss mpjpe` command.

Bounds.
  Layout (UNIT, integers): vertices are multiples of 8 up to 512, weights multiples of 1/8, the ground truth whole multiples of 1000 mm
  chosen so that every residual is an integer triple with an integer norm: every product and every sum is an integer below 2^53 and
  every square root is exact, so A_i equals the gathered sub-block of jrr_jfit_moments' M in bits and b_i and the scalars equal int64
  arithmetic.
  INV against the restatement.  Let d be the largest distance, per array (A_i, b_i, each scalar), between the restatement in float64 and
  the same restatement in extended precision (64-bit mantissa): what float64 arithmetic in ANOTHER order costs on these inputs, the
  ill-conditioned steps (r from sums of K terms, 1 / rho next to a zero residual) included.  Beyond that the device adds the rounding
  of its own sums: an element of A_i or b_i is a sum of 3 count products, each of three factors (w p_a p_b; w carries the rounding of
  a K-term sum, a square root and a division), so |got - exact| <= 3 d + (3 count + K + 8) 2^-53 sum |terms| elementwise, and a scalar,
  a sum of count terms of one sign, 3 d + (count + 8) 2^-53 its value.
  MPJPE consistency: three times the distance between the float32 and the float64 restatement on the same inputs, plus 1e-7 (mm).

Shapes: ns = 4, 21, 62, 83 and counts 1, 3, 63, 64, 65, 2200 from a row that is not 0 (one chunk short of, at and beyond the 64 rows of a
chunk; 35 chunks); K from 2 to 256, i.e. 1 to 153 items a joint, below and above the 16 items of a workgroup, and 1, 4 and 16 lanes per
residual."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jnorm_cases as nc
import jsolve_cases as jc
from conftest import PKG_NAME, ROOT

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
DELTA = 1e-5
U = 2.0 ** -53


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _fit_of(J, rows):
    fit = _mod('engine').RegressorFit(T(J).to(DEV), None, len(rows))
    W = fit.ns + 17
    assert rows.shape[1:] == (W, 3)
    fit.cache[:, :3 * W] = T(np.ascontiguousarray(rows.reshape(len(rows), 3 * W))).to(DEV)
    return fit


def _case_fit(c):
    """a RegressorFit whose lists are the case's (a state prepared from ones on them) and whose cache rows are the case's"""
    fit = _fit_of(nc.pattern(c['lists'], nc.columns(c['ns'])), c['rows'])
    assert fit.ns == c['ns'] and fit.counts == [l.size for l in c['lists']]
    return fit


def _blocks(fit, x, mode, delta, begin=0, count=None):
    return _mod('regressor_solve').parse_norm_blocks(fit.norm_moments(x, mode, delta, begin, count).cpu().numpy(), fit.counts)


# ---- 1. layout and exactness ----
RANGES = ((5, 1), (7, 3), (2, 63), (1, 64), (3, 65), (9, 2200))


@pytest.mark.parametrize('ns', [4, 21, 62, 83])
def test_unit_blocks_of_integers_are_exact(ns):
    J, cols = jc.regressor_with_union(ns)
    lists = jc.lists_of(J, cols)
    rows, x, r = nc.integer_case(ns, 2210, lists, 40 + ns)
    fit = _fit_of(J, rows)
    assert fit.ns == ns and fit.counts == [l.size for l in lists]
    P = rows[:, :ns].astype(np.int64)
    for begin, count in RANGES:
        got = _blocks(fit, x, nc.UNIT, 0.0, begin, count)
        M = fit.moments(begin, count).cpu().numpy()
        sl = slice(begin, begin + count)
        for i in range(1, 17):
            pts = np.concatenate([lists[i], lists[0]])
            A, b = got[i]['A'], got[i]['b']
            assert np.array_equal(A.view(np.uint64), M[np.ix_(pts, pts)].view(np.uint64)), (ns, begin, count, i)
            assert np.array_equal(A.view(np.uint64), A.T.copy().view(np.uint64))
            want_b = np.einsum('sc,sac->a', r[sl, i], P[sl][:, pts])
            norms = np.sqrt((r[sl, i] ** 2).sum(1).astype(np.float64))
            assert (norms == np.round(norms)).all()
            assert np.array_equal(b, want_b.astype(np.float64)), (ns, begin, count, i)
            assert (got[i]['rho'], got[i]['abs'], got[i]['w'], got[i]['n']) == (norms.sum(), norms.sum(), float(count), float(count))
    fit.info()


# ---- 2. INV against the restatement ----
def _check_against_restatement(got, ref, wide, count, what):
    worst = {'A': 0.0, 'b': 0.0, 's': 0.0}
    dist = {'A': 0.0, 'b': 0.0, 's': 0.0}
    for i in range(1, 17):
        K = ref[i]['A'].shape[0]
        assert got[i]['A'].shape == (K, K) and got[i]['n'] == (count if K else 0)
        for k, mag in (('A', 'magA'), ('b', 'magb')):
            if K == 0:
                continue
            exact = np.asarray(wide[i][k])
            d = float(np.abs(np.asarray(ref[i][k], dtype=nc.WIDE) - exact).max())
            bound = 3.0 * d + (3 * count + K + 8) * U * ref[i][mag]
            err = np.abs(got[i][k].astype(nc.WIDE) - exact).astype(np.float64)
            worst[k] = max(worst[k], float((err / np.maximum(bound, 1e-300)).max()))
            dist[k] = max(dist[k], float((err / np.maximum(ref[i][mag], 1e-300)).max()))
            assert (err <= bound).all(), (what, i, k, float((err / bound).max()))
        for k in ('rho', 'abs', 'w'):
            exact = wide[i][k]
            d = abs(float(nc.WIDE(ref[i][k]) - exact))
            bound = 3.0 * d + (count + 8) * U * float(ref[i][k])
            err = abs(float(nc.WIDE(got[i][k]) - exact))
            if K:
                worst['s'] = max(worst['s'], err / bound)
                dist['s'] = max(dist['s'], err / float(ref[i][k]))
            assert err <= bound, (what, i, k, err, bound)
        assert np.array_equal(got[i]['A'].view(np.uint64), got[i]['A'].T.copy().view(np.uint64))
    print(f'{what}: worst share of the bound A {worst["A"]:.3f}, b {worst["b"]:.3f}, scalars {worst["s"]:.3f}; largest distance relative to the '
          f'sum of the terms\' magnitudes A {dist["A"]:.2e}, b {dist["b"]:.2e}, scalars {dist["s"]:.2e}')


@pytest.mark.parametrize('name', ['shipped', 'empty_row', 'empty_pelvis', 'wide'])
def test_inv_blocks_against_the_restatement(name):
    c = nc.table(name)
    fit = _case_fit(c)
    begin, count = 3, c['n'] - 3
    rows = c['rows'][begin:]
    for x, what in ((c['x0'], 'x0'), (nc.random_feasible(np.random.RandomState(6), c['lists']), 'random')):
        got = _blocks(fit, x, nc.INV, DELTA, begin, count)
        ref, wide = nc.blocks(rows, c['lists'], x, nc.INV, DELTA), nc.blocks(rows, c['lists'], x, nc.INV, DELTA, nc.WIDE)
        _check_against_restatement(got, ref, wide, count, f'{name} {what}')
    if name == 'shipped':                                              # the zero residual alone: w = 1 / delta exactly, rho = delta
        one = _blocks(fit, c['x0'], nc.INV, DELTA, 3, 1)[2]
        assert one['abs'] == 0.0 and one['rho'] == DELTA and one['w'] == 1.0 / DELTA and not one['b'].any()
    fit.info()


# ---- 3. repeatability and refusals ----
def test_repeatability_and_the_empty_range():
    c = nc.table('shipped')
    fit = _case_fit(c)
    for mode in (nc.UNIT, nc.INV):
        a, b = fit.norm_moments(c['x0'], mode, DELTA, 3, 147), fit.norm_moments(c['x0'], mode, DELTA, 3, 147)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.isfinite(a).all()
        z = fit.norm_moments(c['x0'], mode, DELTA, 9, 0)
        assert z.numel() == a.numel() and not z.any()
    fit.info()


def test_argument_checks():
    lib_mod, em = _mod('_lib'), _mod('engine')
    lib = lib_mod.load()
    c = nc.table('shipped')
    fit = _case_fit(c)
    n = c['n']
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    counts = (ctypes.c_int32 * 17)(*fit.counts)
    need = ctypes.c_size_t(0)
    nbytes = lib.jrr_jfit_norm_bytes(counts, ctypes.byref(need))
    assert nbytes == 8 * _mod('regressor_solve').norm_block_offsets(fit.counts)[-1] and need.value >= 17 * 256 * 8
    assert lib.jrr_jfit_norm_bytes(counts, None) == nbytes and lib.jrr_jfit_norm_bytes(None, ctypes.byref(need)) == 0 and need.value == 0
    for bad_count in (-1, 129):
        cs = (ctypes.c_int32 * 17)(*fit.counts)
        cs[5] = bad_count
        assert lib.jrr_jfit_norm_bytes(cs, ctypes.byref(need)) == 0 and need.value == 0
    lib.jrr_jfit_norm_bytes(counts, ctypes.byref(need))
    sb = need.value
    x = torch.zeros(17, 128, dtype=torch.float64, device=DEV)
    for i, r in enumerate(c['x0']):
        x[i, :r.size] = T(r)
    out = torch.zeros(nbytes // 8, dtype=torch.float64, device=DEV)
    scratch = torch.zeros(sb // 8, dtype=torch.float64, device=DEV)
    state0 = fit.state.clone()
    call = lambda st, ca, n_rows, begin, count, ns, xx, mode, delta, o, sc, nb: lib.jrr_jfit_norm_moments(st, ca, n_rows, begin, count, ns, xx, mode,
                                                                                                         delta, o, sc, nb, None)
    S, C, X, O, W = P(fit.state), P(fit.cache), P(x), P(out), P(scratch)
    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    assert call(S, C, n, 0, n, 62, X, 1, DELTA, O, W, sb) == 0
    assert call(S, C, n, 0, n, 62, X, 0, 0.0, O, W, sb) == 0            # UNIT takes delta = 0
    bad = [
        call(None, C, n, 0, n, 62, X, 1, DELTA, O, W, sb), call(S, None, n, 0, n, 62, X, 1, DELTA, O, W, sb),
        call(S, C, n, 0, n, 62, None, 1, DELTA, O, W, sb), call(S, C, n, 0, n, 62, X, 1, DELTA, None, W, sb),
        call(S, C, n, 0, n, 62, X, 1, DELTA, O, None, sb),
        call(S, off(fit.cache, 4), n, 0, n, 62, X, 1, DELTA, O, W, sb), call(S, C, n, 0, n, 62, off(x, 4), 1, DELTA, O, W, sb),
        call(S, C, n, 0, n, 62, X, 1, DELTA, off(out, 4), W, sb), call(S, C, n, 0, n, 62, X, 1, DELTA, O, off(scratch, 4), sb),
        call(S, C, n, -1, 10, 62, X, 1, DELTA, O, W, sb), call(S, C, n, 0, n + 1, 62, X, 1, DELTA, O, W, sb),
        call(S, C, n, 100, n - 99, 62, X, 1, DELTA, O, W, sb), call(S, C, n, n + 1, 0, 62, X, 1, DELTA, O, W, sb),
        call(S, C, n, 0, -1, 62, X, 1, DELTA, O, W, sb), call(S, C, -1, 0, 0, 62, X, 1, DELTA, O, W, sb),
        call(S, C, n, 0, n, 0, X, 1, DELTA, O, W, sb), call(S, C, n, 0, n, 2177, X, 1, DELTA, O, W, sb),
        call(S, C, n, 0, n, 62, X, 2, DELTA, O, W, sb), call(S, C, n, 0, n, 62, X, -1, DELTA, O, W, sb),
        call(S, C, n, 0, n, 62, X, 1, 0.0, O, W, sb), call(S, C, n, 0, n, 62, X, 1, -DELTA, O, W, sb),
        call(S, C, n, 0, n, 62, X, 1, float('inf'), O, W, sb), call(S, C, n, 0, n, 62, X, 1, float('nan'), O, W, sb),
        call(S, C, n, 0, n, 62, X, 0, -DELTA, O, W, sb), call(S, C, n, 0, n, 62, X, 0, float('nan'), O, W, sb),
    ]
    assert bad == [-1] * len(bad), bad
    assert b'jrr_jfit_norm_moments' in lib.jrr_last_error()
    assert call(S, C, n, 0, n, 62, X, 1, DELTA, O, W, sb - 8) == -3 and b'jrr_jfit_norm_bytes' in lib.jrr_last_error()
    torch.cuda.synchronize()
    assert torch.equal(fit.state, state0)                               # no call touched the state
    fit.info()
    # a foreign ns is found on the device: NaN everywhere, the error word, nothing else
    assert call(S, C, n, 0, n, 61, X, 1, DELTA, O, W, sb) == 0
    assert torch.isnan(out).all()
    with pytest.raises(lib_mod.JrrError, match='not the prepared one'):
        fit.info()
    assert em.NORM_UNIT == 0 and em.NORM_INV == 1


# ---- 4. the MPJPE it states is jrr_evaluate's ----
def _normalised32(x):
    """what jrr_jfit_set_entries makes of raw float32 values: relu over the float32 of their float64 sum"""
    out = []
    for r in x:
        r32 = np.asarray(r, dtype=np.float32)
        out.append(r32 / np.float32(r32.astype(np.float64).sum()) if r32.size else r32)
    return out


def _mpjpe_bound(rows, lists, jn):
    """the project's rule (jfit_cases.bound): three times the largest distance between the float32 and the float64 restatement, plus
    1e-7 -- taken over the restated distances per (row, joint), in mm, BEFORE the mean: the means of the two restatements agree far
    better than any single distance does (the float32 errors of 10 000 distances cancel), and a mean errs by no more than its terms"""
    e64, e32 = nc.joint_errors_mm(rows, lists, jn), nc.joint_errors_mm(rows, lists, jn, np.float32)
    return 3.0 * float(np.abs(e32.astype(np.float64) - e64).max()) + 1e-7


def _device_mpjpe(fit, lists, cols, x32, begin, count):
    J = np.zeros((17, nc.V), dtype=np.float32)
    for i, l in enumerate(lists):
        J[i, cols[l]] = x32[i]
    fit.set_entries(T(J).to(DEV))
    err, _ = _mod('engine').evaluate(fit.joints(begin, count), fit.ground_truth_mm(begin, count))
    return float(err.double().mean().item()) * 1000.0


@pytest.mark.parametrize('name', ['shipped', 'planted'])
def test_the_objective_is_the_mpjpe_of_evaluate(name):
    c = nc.table(name)
    fit = _case_fit(c)
    n, lists = c['n'], c['lists']
    x32 = [np.asarray(r, dtype=np.float32) for r in nc.random_feasible(np.random.RandomState(8), lists)]
    jn = _normalised32(x32)
    want = _device_mpjpe(fit, lists, nc.columns(c['ns']), x32, 0, n)
    bl = _blocks(fit, [r.astype(np.float64) for r in jn], nc.INV, DELTA, 0, n)
    got = 1000.0 * _mod('regressor_solve').norm_objective(bl, n)[1]
    m64, m32 = nc.mpjpe_mm(c['rows'], lists, jn), nc.mpjpe_mm(c['rows'], lists, jn, np.float32)
    bound = _mpjpe_bound(c['rows'], lists, jn)
    print(f'{name}: {got:.9f} mm from the pass, {want:.9f} mm from jrr_jfit_joints + jrr_evaluate, {m64:.9f} restated (float32 {m32:.9f}): '
          f'distance {abs(got - want):.3e}, bound {bound:.3e}')
    assert abs(got - want) <= bound
    fit.info()


# ---- 5. the solve with device passes ----
def test_the_solve_with_device_passes():
    rs = _mod('regressor_solve')
    c = nc.table('planted')
    fit = _case_fit(c)
    n, lists = c['n'], c['lists']
    seen = []

    def device_pass(x, mode, delta):
        seen.append(([r.copy() for r in x], mode))
        return _blocks(fit, x, mode, delta, 0, n)

    r = rs.solve_norm(device_pass, n, lists, c['x0'], DELTA, tol=1e-6, max_iter=400)
    cpu = rs.solve_norm(lambda x, mode, delta: rs.norm_blocks_reference(c['rows'], lists, x, mode, delta), n, lists, c['x0'], DELTA, tol=1e-6,
                        max_iter=400)
    seq, o = np.asarray(r['sequence']), r['objective']
    worst = lambda x: max(float(np.abs(a - b).max()) for a, b in zip(x, c['x_true']))
    print(f'device passes: MPJPE {1e3 * o["start"]:.4f} -> {1e3 * o["mse"]:.4f} -> {1e3 * o["final"]:.4f} mm, gap {1e3 * r["gap"]:.2e} mm, {r["passes"]} '
          f'passes; worst weight error {worst(r["x_mse"]):.4f} (MSE) against {worst(r["x"]):.4f}; the host-driven solve ends at '
          f'{1e3 * cpu["objective"]["final"]:.9f} against {1e3 * o["final"]:.9f} mm')
    assert r['converged'] and (np.diff(seq) <= 1e-13 * seq[:-1]).all()
    assert o['final'] <= o['mse'] + r['gap'] + DELTA
    assert worst(r['x']) < worst(r['x_mse'])
    # the objective sequence against the host's pass at the same points, to the scalar bound of test 2
    inv = [x for x, mode in seen if mode == nc.INV]
    assert len(inv) == len(seq)
    for x, Ld in zip(inv, seq):
        ref, wide = (sum(b['rho'] for b in nc.blocks(c['rows'], lists, x, nc.INV, DELTA, dt)[1:]) for dt in (np.float64, nc.WIDE))
        # (16 scalars, each within 3 d_i + (n + 8) U of its value, added on the host: 16 more roundings; two for the mean)
        bound = (3.0 * abs(float(nc.WIDE(ref) - wide)) + (n + 8 + 16) * U * float(ref)) / (n * 17)
        assert abs(float(nc.WIDE(Ld) * (n * 17) - wide)) / (n * 17) <= bound + 2 * U * Ld
    # both solves end within their gaps of the same optimum
    assert abs(r['smoothed']['final'] - cpu['smoothed']['final']) <= max(r['gap'], cpu['gap'])
    fit.info()


# ---- 6. the command ----
N_CMD = 64


@pytest.fixture(scope='module')
def command_runs(tmp_path_factory, smpl_model_np):
    """64 synthetic meshes in the --eval_vertices format, the MPJPE solve on them with --fit_rings 0 and 1, and the evaluation of a
    checkpoint"""
    em, sm = _mod('engine'), _mod('smpl_model')
    root = str(tmp_path_factory.mktemp('norm_solve_data'))
    J_np = sm.default_h36m_regressor('/nonexistent', allow_default=True)
    full = sm.synthetic_batch(smpl_model_np, J_np, N_CMD, seed=6)
    paths = [f'/data/h36m/S9/Act{(i // 16) // 2} 1/imageSequence/{(i // 16) % 2 + 1}/img_{5 * (i % 16 + 1):06d}.jpg' for i in range(N_CMD)]
    x6d, betas = (T(full[k]).to(DEV).contiguous() for k in ('pose6d', 'betas'))
    eng = em.RefineEngine(em.DeviceModel(smpl_model_np, DEV), N_CMD, flags=em.FLAG_KEEP_VERTS)
    eng.set_j_regressor(T(J_np))
    _, verts = eng.find_joints_forward(betas, x6d=x6d, return_verts=True)
    verts = verts.cpu().numpy()
    rng = np.random.RandomState(12)
    other = np.where(J_np > 0, J_np * rng.uniform(0.3, 3.0, size=J_np.shape), 0)
    other = other / other.sum(1, keepdims=True)
    gt = np.einsum('jv,bvc->bjc', other, verts.astype(np.float64)) * 1000.0 + rng.normal(0, 2.0, size=(N_CMD, 17, 3))
    gt[::9] += rng.normal(0, 150.0, size=gt[::9].shape)                 # badly fitted frames
    gt = gt.astype(np.float32)
    vdir = os.path.join(root, 'meshes')
    os.makedirs(vdir)
    np.save(os.path.join(vdir, 'vertices.npy'), verts)
    np.save(os.path.join(vdir, 'gt_j3d.npy'), gt)
    with open(os.path.join(vdir, 'paths.txt'), 'w') as f:
        f.write('\n'.join(paths) + '\n')
    torch.cuda.synchronize()
    common = ['--synthetic', '--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent', '--device', DEV, '--batch_size', '32']
    outs = {}
    for rings in (0, 1):
        out = os.path.join(root, f'solve_{rings}')
        cmd = [sys.executable, os.path.join(ROOT, 'main.py'), '--fit_regressor', out, '--fit_solve', '--fit_solve_loss', 'mpjpe', '--fit_rings',
               str(rings), '--fit_holdout', '0.25', '--fit_from', vdir] + common
        r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs[rings] = (out, r.stdout)
    rep = os.path.join(root, 'report')
    cmd = [sys.executable, os.path.join(ROOT, 'main.py'), '--eval_vertices', vdir, '--eval_report', rep, '--eval_j_regressor',
           os.path.join(outs[1][0], 'retrained_J_Regressor.pt')] + common
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return outs, rep, J_np, verts, gt, paths


@pytest.mark.parametrize('rings', [0, 1])
def test_the_mpjpe_solve_command(command_runs, rings):
    outs, rep, J_np, verts, gt, paths = command_runs
    rs, rf, checkpoint = _mod('regressor_solve'), _mod('regressor_fit'), _mod('checkpoint')
    out, stdout = outs[rings]
    assert sorted(os.listdir(out)) == ['retrained_J_Regressor.pt', 'solve.json']
    with open(os.path.join(out, 'solve.json')) as f:
        doc = json.load(f)
    assert sorted(doc) == sorted(rs.SOLVE_KEYS + ('norm',))
    norm = doc['norm']
    assert sorted(norm) == sorted(rs.NORM_KEYS) and sorted(norm['objective_mm']) == sorted(rs.NORM_OBJECTIVE_KEYS)
    o = norm['objective_mm']
    lines = [l for l in stdout.splitlines() if l.startswith('solved the regressor on ')]
    assert len(lines) == 1 and 'MSE optimum' in lines[0] and 'above the optimum' in lines[0] and lines[0].endswith('retrained_J_Regressor.pt')
    print(rings, 'objective', o, 'gap', norm['gap_mm'], 'bound', norm['bound_mm'], 'passes', norm['passes'], 'inner', norm['inner_iterations'],
          'loss', doc['loss'], 'MPJPE', doc['initial']['train']['mpjpe_mm'], '->', doc['final']['train']['mpjpe_mm'])
    assert norm['delta_mm'] == 0.01 and norm['bound_mm'] == pytest.approx(norm['gap_mm'] + 0.01, rel=1e-12) and norm['passes'] >= 2
    assert o['final'] <= o['mse'] + norm['bound_mm']
    assert all(o[k] is not None and o[k] > 0 for k in rs.NORM_OBJECTIVE_KEYS)
    assert doc['loss']['train_after'] <= doc['loss']['train_before'] and doc['flags']['fit_solve_loss'] == 'mpjpe'
    # the score of the checkpoint's fp32 weights against the objective at the solved weights: the bound of test 4 on these inputs
    held = rf.holdout_split(N_CMD, 0.25, paths)
    assert doc['rows'] == {'train': int((~held).sum()), 'holdout': int(held.sum())} and held.any()
    J = checkpoint.load_j_regressor(os.path.join(out, 'retrained_J_Regressor.pt')).numpy()
    cands = rs.ring_candidates(J_np, _mod('smpl_model').synthetic_smpl(1234)['faces'], rings)
    cols = np.unique(np.concatenate(cands))
    lists = [np.searchsorted(cols, v) for v in cands]
    jn = _normalised32([np.maximum(J[i, v], 0) for i, v in enumerate(cands)])
    centred = gt - gt[:, :1]
    rows = np.concatenate([verts[:, cols], centred], axis=1)[~held]
    m64, m32 = nc.mpjpe_mm(rows, lists, jn), nc.mpjpe_mm(rows, lists, jn, np.float32)
    bound = _mpjpe_bound(rows, lists, jn)
    print(f'rings {rings}: final.train.mpjpe_mm {doc["final"]["train"]["mpjpe_mm"]:.9f}, objective_mm.final {o["final"]:.9f}, restated {m64:.9f} '
          f'(float32 {m32:.9f}), bound {bound:.3e}')
    assert abs(doc['final']['train']['mpjpe_mm'] - o['final']) <= bound
    assert J.shape == (17, 6890) and doc['support']['after'] == [int(c) for c in (J > 0).sum(1)]


def test_the_evaluation_accepts_the_checkpoint(command_runs):
    outs, rep = command_runs[0], command_runs[1]
    assert sorted(os.listdir(rep)) == ['eval.json', 'eval.md']
    doc = _mod('eval_report').load(rep)
    assert doc['j_regressor_retrained']['path'].endswith('retrained_J_Regressor.pt')
