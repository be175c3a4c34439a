"""Inputs and the restatement for the MPJPE solve of the regressor fit (`--fit_solve --fit_solve_loss mpjpe`; regressor_solve.py,
include/jrr.h jrr_jfit_norm_moments), shared by tests/test_regressor_norm_solve.py (CPU) and tests/test_gpu_regressor_norm_solve.py.

The restatement (`blocks`) is the definition written out joint by joint, in the arithmetic asked for: float64, or numpy's extended
precision where the host has it (x86: 64-bit mantissa), which the rounding bounds of the GPU tests are measured against.

Cases (`table`):
  planted   600 rows on a 40-vertex union, 17 rows of 5 entries, weights planted, 5 mm of noise on the ground truth and on every tenth
            row a further N(0, 200 mm) on every joint: the rows a squared loss lets decide the weights
  clean     the same without noise and outliers
  shipped   counts like the shipped regressor's, rows 1 and 2 sharing vertices with the pelvis row; one residual exactly zero (row 2 and the
            pelvis row carry dyadic weights and, in row 3 of the table, vertices on a grid of 1/8 m), one gross outlier
  empty_row / empty_pelvis   a joint row, or the pelvis row, without entries
  wide      row 1 of 128 entries against a pelvis row of 128 (K = 256; 40 vertices shared), 230 union vertices
"""
import numpy as np

NJ, V = 17, 6890
UNIT, INV = 0, 1
WIDE = np.longdouble if np.finfo(np.longdouble).eps < 2.0 ** -60 else np.float64

_CACHE = {}


def _cover(rng, ns, sizes):
    """lists of the given sizes over 0 .. ns - 1 that together use every vertex: slots of shuffled copies of the union"""
    need = sum(sizes)
    pool = np.concatenate([rng.permutation(ns) for _ in range(need // ns + 2)])
    lists, at = [], 0
    for s in sizes:
        l = []
        while len(l) < s:
            if pool[at] not in l:
                l.append(int(pool[at]))
            at += 1
        lists.append(np.sort(np.asarray(l, dtype=np.int64)))
    used = np.unique(np.concatenate(lists)) if need else np.zeros(0, dtype=np.int64)
    assert used.size == ns or need < ns
    return lists


def _joints(points, lists, x):
    P = points.astype(np.float64)
    n = P.shape[0]
    return np.stack([np.einsum('e,nec->nc', x[i], P[:, lists[i]]) if lists[i].size else np.zeros((n, 3)) for i in range(NJ)], axis=1)


def _dirichlet(rng, lists):
    return [rng.dirichlet(np.ones(l.size)) if l.size else np.zeros(0) for l in lists]


def _dyadic(rng, k):
    """k positive multiples of 1/16 that sum to 1 (k <= 16)"""
    w = np.ones(k)
    for _ in range(16 - k):
        w[rng.randint(k)] += 1
    return w / 16.0


def table(name):
    """dict: rows (n, ns + 17, 3) float32 -- the cache rows as points: the union's vertices in m, then the ground truth in mm; lists;
    x0 (the start), x_true (what generated the ground truth), n, ns"""
    if name in _CACHE:
        return _CACHE[name]
    if name in ('planted', 'clean'):
        rng = np.random.RandomState(20)
        n, ns = 600, 40
        lists = _cover(rng, ns, [5] * NJ)
        points = (rng.normal(0, 1, size=(n, ns, 3)) * np.array([0.15, 0.45, 0.1])).astype(np.float32)
        x_true = _dirichlet(rng, lists)
        j = _joints(points, lists, x_true)
        gt = (j - j[:, :1]) * 1000.0
        noise, gross = rng.normal(0, 5.0, size=gt.shape), rng.normal(0, 200.0, size=gt.shape) * (rng.uniform(size=(n, 1, 1)) < 0.1)
        if name == 'planted':
            gt = gt + noise + gross
        gt[:, 0] = 0.0
        x0 = [np.full(l.size, 1.0 / l.size) for l in lists]
    else:
        seed, n, sizes, ns = {'shipped': (21, 150, (5, 9, 2, 3, 4, 1, 6, 3, 2, 4, 5, 3, 2, 3, 4, 7, 12), 62),
                              'empty_row': (22, 70, (4, 6, 2, 3, 0, 1, 5, 3, 2, 4, 3, 3, 2, 3, 4, 5, 8), 50),
                              'empty_pelvis': (23, 70, (0, 6, 2, 3, 4, 1, 5, 3, 2, 4, 3, 3, 2, 3, 4, 5, 8), 50),
                              'wide': (24, 70, (128, 128, 2, 3, 40, 1, 6, 3, 2, 4, 5, 3, 2, 3, 4, 7, 12), 230)}[name]
        rng = np.random.RandomState(seed)
        lists = _cover(rng, ns, sizes)
        if name == 'shipped':                                          # rows 1 and 2 share vertices with the pelvis row
            lists[1] = np.unique(np.concatenate([lists[1], lists[0][:2]]))
            lists[2] = np.unique(np.concatenate([lists[2], lists[0][1:2]]))
        if name == 'wide':                                             # 40 of row 1's vertices are the pelvis row's
            rest = np.setdiff1d(np.arange(ns), lists[0])
            lists[1] = np.sort(np.concatenate([lists[0][:40], rest[:88]]))
            lists[4] = np.sort(rest[62:102])
            assert np.unique(np.concatenate(lists)).size == ns
        points = (rng.normal(0, 1, size=(n, ns, 3)) * np.array([0.15, 0.45, 0.1]) + rng.normal(0, 0.3, size=(n, 1, 3))).astype(np.float32)
        x_true, x0 = _dirichlet(rng, lists), _dirichlet(rng, lists)
        if name == 'shipped':
            x0[0], x0[2] = _dyadic(rng, lists[0].size), _dyadic(rng, lists[2].size)
            on = np.union1d(lists[0], lists[2])
            points[3, on] = rng.randint(-16, 17, size=(on.size, 3)) / 8.0
        j = _joints(points, lists, x_true)
        gt = (j - j[:, :1]) * 1000.0 + rng.normal(0, 8.0, size=j.shape)
        gt[:, 0] = 0.0
        if name == 'shipped':
            j0 = _joints(points[3:4], lists, x0)[0]
            gt[3, 2] = (j0[2] - j0[0]) * 1000.0                       # multiples of 125 mm: the residual of (row 3, joint 2) at x0 is exactly 0
            gt[5, 3] += 5000.0                                         # a gross outlier
    out = {'rows': np.concatenate([points, gt.astype(np.float32)], axis=1), 'lists': lists, 'x0': x0, 'x_true': x_true, 'n': n, 'ns': ns}
    if name == 'shipped':
        assert (out['rows'][3, ns + 2] == gt[3, 2]).all()
    _CACHE[name] = out
    return out


def blocks(rows, lists, x, mode, delta, dtype=np.float64):
    """the pass restated: list of 17, None for the pelvis, else {'A', 'b', 'rho', 'abs', 'w', 'n', 'cnt'}, everything in `dtype`;
    and beside it 'magA' / 'magb': the sums of the terms' magnitudes, w |p_a||p_b| and w |r||p_a|, which rounding bounds are stated in"""
    R = np.asarray(rows).astype(dtype)
    n, ns = R.shape[0], R.shape[1] - NJ
    out = [None]
    d = dtype(delta)
    for i in range(1, NJ):
        ci = len(lists[i])
        if ci == 0:
            out.append({'A': np.zeros((0, 0), dtype), 'b': np.zeros(0, dtype), 'rho': dtype(0), 'abs': dtype(0), 'w': dtype(0), 'n': 0.0, 'cnt': 0,
                        'magA': np.zeros((0, 0)), 'magb': np.zeros(0)})
            continue
        P = np.concatenate([R[:, lists[i]], R[:, lists[0]]], axis=1)
        wt = np.concatenate([np.asarray(x[i]).astype(dtype), -np.asarray(x[0]).astype(dtype)])
        r = (wt[None, :, None] * P).sum(1) - R[:, ns + i] / dtype(1000.0)
        rr = (r * r).sum(1)
        rho = np.sqrt(rr + d * d)
        w = dtype(1.0) / rho if mode == INV else np.ones(n, dtype)
        wP = w[:, None, None] * P
        A = np.einsum('nac,nbc->ab', wP, P)
        b = np.einsum('nc,nac->a', r, wP)
        out.append({'A': A, 'b': b, 'rho': rho.sum(), 'abs': np.sqrt(rr).sum(), 'w': w.sum(), 'n': float(n), 'cnt': ci,
                    'magA': np.einsum('nac,nbc->ab', np.abs(wP), np.abs(P)).astype(np.float64),
                    'magb': np.einsum('nc,nac->a', np.abs(r), np.abs(wP)).astype(np.float64)})
    return out


def objective(rows, lists, x, delta, dtype=np.float64):
    """(L_delta, L) from the rows themselves"""
    bl = blocks(rows, lists, x, UNIT, delta, dtype)
    n = len(rows)
    return float(sum(b['rho'] for b in bl[1:])) / (n * NJ), float(sum(b['abs'] for b in bl[1:])) / (n * NJ)


def mpjpe_mm(rows, lists, x, dtype=np.float64):
    """the MPJPE jrr_evaluate states for these weights: joints minus the pelvis against the ground truth minus ITS pelvis, the mean of the
    17 distances (an empty row's joint is NaN there and is left out here, as the fit leaves it out; the mean still divides by 17)"""
    return float(joint_errors_mm(rows, lists, x, dtype).astype(np.float64).mean())


def joint_errors_mm(rows, lists, x, dtype=np.float64):
    """(n, 17): the distances behind mpjpe_mm, in the arithmetic asked for (zeros for the pelvis and for a row without entries)"""
    R = np.asarray(rows).astype(dtype)
    n, ns = R.shape[0], R.shape[1] - NJ
    out = np.zeros((n, NJ), dtype)
    j0 = (np.asarray(x[0]).astype(dtype)[None, :, None] * R[:, lists[0]]).sum(1) if len(lists[0]) else np.zeros((n, 3), dtype)
    for i in range(1, NJ):
        if len(lists[i]):
            j = (np.asarray(x[i]).astype(dtype)[None, :, None] * R[:, lists[i]]).sum(1)
            dv = (j - j0) * dtype(1000.0) - (R[:, ns + i] - R[:, ns])
            out[:, i] = np.sqrt((dv * dv).sum(1))
    return out


def random_feasible(rng, lists):
    return [rng.dirichlet(np.full(len(l), rng.choice([0.3, 1.0, 4.0]))) if len(l) else np.zeros(0) for l in lists]


def pattern(lists, cols):
    """(17, 6890) float32: ones on the lists' vertices -- what a device state with exactly these lists is prepared from"""
    J = np.zeros((NJ, V), dtype=np.float32)
    for i, l in enumerate(lists):
        J[i, cols[l]] = 1.0
    return J


def columns(ns, seed=9):
    return np.sort(np.random.RandomState(seed).choice(V, ns, replace=False))


# ---- integers for the layout test: every product and every sum is an integer below 2^53, and every |r| is one too ----------------------
_QUADS = np.array([(1, 2, 2), (2, 3, 6), (0, 3, 4), (0, 0, 5), (1, 4, 8), (4, 4, 7), (2, 6, 9), (6, 6, 7), (0, 0, 0), (3, 4, 12)], dtype=np.int64)


def integer_case(ns, n, lists, seed):
    """rows (n, ns + 17, 3) float32: vertices multiples of 8 in [-512, 512] m, weights multiples of 1/8, and a ground truth in whole
    multiples of 1000 mm chosen so that every residual is a signed permutation of a triple with an integer norm.  Returns (rows, x,
    r (n, 17, 3) int64: the residuals; r[:, 0] unused)"""
    rng = np.random.RandomState(seed)
    v = 8 * rng.randint(-64, 65, size=(n, ns, 3)).astype(np.int64)
    x8 = [rng.randint(1, 9, size=len(l)).astype(np.int64) for l in lists]
    q = np.stack([(x8[i][None, :, None] * v[:, lists[i]]).sum(1) // 8 for i in range(NJ)], axis=1)      # exact: v is a multiple of 8
    r = _QUADS[rng.randint(len(_QUADS), size=(n, NJ))]
    r = np.take_along_axis(r, np.argsort(rng.uniform(size=(n, NJ, 3)), axis=2), axis=2) * rng.choice([-1, 1], size=(n, NJ, 3))
    gt = (q - q[:, :1] - r) * 1000
    assert np.abs(gt).max() < 2 ** 24
    rows = np.concatenate([v, gt], axis=1).astype(np.float32)
    return rows, [w / 8.0 for w in x8], r
