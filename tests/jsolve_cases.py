"""Inputs and the float64 restatement for the exact solve of the regressor fit (`--fit_solve`; regressor_solve.py, include/jrr.h
jrr_jfit_moments / jrr_jfit_set_entries), shared by tests/test_regressor_solve.py (CPU) and tests/test_gpu_regressor_solve.py.

The restatement is the definition written out: `moments` is X^T X over the rows' points in float64 (or int64 for integer inputs),
`direct_loss` is the mean over the rows of (x_i . v - x_0 . v - gt / 1000)^2 without any moments.

Cases (`table`): clusters of vertices a few centimetres across around 17 body-scale centres, turned and deformed per sample, with
millimetres of per-vertex jitter -- neighbouring vertices are nearly parallel, so the Gram matrix is ill-conditioned as on a body --
and ground truth from ANOTHER simplex regressor on the candidate lists (some of its entries at zero, some on candidates the initial
regressor does not use), with noise or, `planted`, without.  Every case names its support (the initial regressor's positive entries,
`lists0`) and its candidate lists (`lists1`: the support plus further vertices of the cluster, the initial weight zero there).
"""
import numpy as np

NJ, V = 17, 6890
TOL = 1e-6
MAX_ITER = 400

# name -> (seed, rows, entries per row of the support, further candidates per row, noise in mm)
CASES = {
    'body': (3, 240, (5, 9, 2, 3, 4, 1, 6, 3, 2, 4, 5, 3, 2, 3, 4, 7, 12), 4, 8.0),
    'empty_row': (4, 160, (4, 6, 2, 3, 0, 1, 5, 3, 2, 4, 3, 3, 2, 3, 4, 5, 8), 3, 8.0),
    'empty_pelvis': (5, 160, (0, 6, 2, 3, 4, 1, 5, 3, 2, 4, 3, 3, 2, 3, 4, 5, 8), 3, 8.0),
    'few_rows': (6, 9, (5, 9, 2, 3, 4, 1, 6, 3, 2, 4, 5, 3, 2, 3, 4, 7, 30), 5, 8.0),      # 27 equations per joint: singular Gram blocks
    'planted': (7, 200, (5, 9, 2, 3, 4, 1, 6, 3, 2, 4, 5, 3, 2, 3, 4, 7, 12), 4, 0.0),
}


def _rotations(rng, n, scale):
    """n rotation matrices about random axes, angles of standard deviation `scale` rad (Rodrigues)"""
    w = rng.normal(0, scale, size=(n, 3))
    th = np.linalg.norm(w, axis=1)[:, None, None]
    k = w / np.maximum(np.linalg.norm(w, axis=1, keepdims=True), 1e-12)
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


_CACHE = {}


def table(name):
    """dict: points (n, ns, 3) float32 the union's vertices in m; gt (n, 17, 3) float32 pelvis-centred mm; lists0 / lists1: per row the
    positions in the union of the support / of the candidates (ascending); x0: the initial weights on lists0; x0_1: the same on lists1
    (zeros on the further candidates); x_true: the generating weights on lists1; n, ns"""
    if name in _CACHE:
        return _CACHE[name]
    seed, n, counts, extra, noise_mm = CASES[name]
    rng = np.random.RandomState(seed)
    sizes = [c + extra if c else 0 for c in counts]
    # the union: cluster i owns sizes[i] vertices; rows 1 and 2 also list two vertices of cluster 0 (when it has any)
    own, start = [], 0
    for s in sizes:
        own.append(np.arange(start, start + s))
        start += s
    ns = start
    centre = rng.normal(0, 1, size=(NJ, 3)) * np.array([0.15, 0.45, 0.1])
    offs = rng.normal(0, 0.03, size=(ns, 3))
    cluster = np.concatenate([np.full(s, i) for i, s in enumerate(sizes)]).astype(np.int64)
    R = _rotations(rng, n, 0.5)
    A = np.eye(3) + rng.normal(0, 0.15, size=(n, NJ, 3, 3))                         # each cluster deforms by itself
    local = np.einsum('nuab,ub->nua', A[:, cluster], offs) + centre[cluster] * (1 + rng.normal(0, 0.05, size=(n, ns, 1)))
    points = np.einsum('nab,nub->nua', R, local) + rng.normal(0, 0.002, size=(n, ns, 3))
    points = points.astype(np.float32)
    lists0, lists1 = [], []
    for i, c in enumerate(counts):
        sup = np.sort(rng.choice(own[i], c, replace=False)) if c else np.zeros(0, dtype=np.int64)
        cand = own[i]
        if i in (1, 2) and counts[0]:
            shared = own[0][:2]
            sup, cand = np.sort(np.concatenate([sup, shared[:1]])), np.sort(np.concatenate([cand, shared]))
        lists0.append(sup.astype(np.int64))
        lists1.append(cand.astype(np.int64))
    x0, x0_1, x_true = [], [], []
    for i in range(NJ):
        w = rng.uniform(0.05, 1.0, size=lists0[i].size)
        x0.append(w / w.sum() if w.size else w)
        full = np.zeros(lists1[i].size)
        full[np.searchsorted(lists1[i], lists0[i])] = x0[i]
        x0_1.append(full)
        t = rng.uniform(0.0, 1.0, size=lists1[i].size) * (rng.uniform(size=lists1[i].size) < 0.6)
        if t.size and t.sum() == 0:
            t[0] = 1.0
        x_true.append(t / t.sum() if t.size else t)
    P = points.astype(np.float64)
    joints = np.stack([np.einsum('e,nec->nc', x_true[i], P[:, lists1[i]]) if lists1[i].size else np.zeros((n, 3)) for i in range(NJ)], axis=1)
    gt = (joints - joints[:, :1]) * 1000.0
    if not lists1[0].size:
        gt = joints * 1000.0                                                         # an empty pelvis row centres on the origin
    gt = gt + rng.normal(0, noise_mm, size=gt.shape) if noise_mm else gt
    for i in range(NJ):
        if not lists1[i].size:
            gt[:, i] = rng.normal(0, 300.0, size=(n, 3))                              # whatever: the row is left out of the loss
    out = {'points': points, 'gt': gt.astype(np.float32), 'lists0': lists0, 'lists1': lists1, 'x0': x0, 'x0_1': x0_1, 'x_true': x_true,
           'n': n, 'ns': ns}
    _CACHE[name] = out
    return out


def rows_of(points, gt):
    """(n, W, 3): a cache row as points -- the union's vertices, then the ground truth"""
    return np.concatenate([np.asarray(points), np.asarray(gt)], axis=1)


def moments(rows, dtype=np.float64):
    """M[w][w'] = sum over rows and axes of row[w][c] * row[w'][c]"""
    X = np.asarray(rows).astype(dtype)
    X = X.transpose(0, 2, 1).reshape(-1, X.shape[1])
    return X.T @ X


def moments_reference(rows):
    """the float64 moments for a rounding bound: summed in extended precision where the host has it (x86: 64-bit mantissa) and rounded
    once, so that the reference's own rounding does not use up the bound the kernel is held to; plain float64 sums elsewhere"""
    wide = np.longdouble if np.finfo(np.longdouble).eps < 2.0 ** -60 else np.float64
    return moments(rows, wide).astype(np.float64)


def abs_moments(rows):
    """sum of |a| |b|: what the rounding bound of a sum of exact products is stated in"""
    return moments(np.abs(np.asarray(rows, dtype=np.float64)))


def direct_loss(points, gt, lists, x):
    """the loss as jrr_jfit_run defines it, from the rows themselves in float64: joints minus joint 0, gt / 1000, the mean over
    n * 51; a row without entries is left out and an empty pelvis row centres on the origin"""
    P, g = np.asarray(points, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    n = P.shape[0]
    j0 = np.einsum('e,nec->nc', x[0], P[:, lists[0]]) if len(lists[0]) else np.zeros((n, 3))
    total = 0.0
    for i in range(NJ):
        if len(lists[i]):
            d = np.einsum('e,nec->nc', x[i], P[:, lists[i]]) - j0 - g[:, i] / 1000.0
            total += float((d * d).sum())
    return total / (n * NJ * 3)


def random_feasible(rng, lists, near=None, scale=0.0):
    """a point of the product of simplices: Dirichlet rows, or `near` perturbed on the simplex"""
    out = []
    for i, l in enumerate(lists):
        k = len(l)
        if k == 0:
            out.append(np.zeros(0))
            continue
        w = rng.dirichlet(np.full(k, rng.choice([0.2, 1.0, 5.0])))
        out.append(w if near is None else (1 - scale) * near[i] + scale * w)
    return out


# ---- a hand-made mesh for ring_candidates: a 4 x 3 grid of vertices 0 .. 11, row-major, two triangles per cell -------------------------
#   0 - 1 - 2 - 3
#   | \ | \ | \ |
#   4 - 5 - 6 - 7
#   | \ | \ | \ |
#   8 - 9 - 10 - 11
GRID_FACES = np.array([(a, a + 5, a + 4) for a in (0, 1, 2, 4, 5, 6)] + [(a, a + 1, a + 5) for a in (0, 1, 2, 4, 5, 6)], dtype=np.int64)


# ---- the GPU side: a regressor whose union has a chosen size, and cache rows of integers or of body-sized numbers ----------------------
def regressor_with_union(ns, seed=0):
    """(J (17,6890) float32, cols (ns,)): every column of `cols` is listed by row (k mod 17), and every row also lists cols[i mod ns],
    so that no row is empty and the union is exactly `cols`"""
    rng = np.random.RandomState(100 + seed + ns)
    cols = np.sort(rng.choice(V, ns, replace=False))
    J = np.zeros((NJ, V), dtype=np.float32)
    for k, c in enumerate(cols):
        J[k % NJ, c] = rng.uniform(0.05, 0.4)
    for i in range(NJ):
        J[i, cols[i % ns]] = rng.uniform(0.05, 0.4)
    return J, cols


def lists_of(J, cols):
    return [np.searchsorted(cols, np.flatnonzero(J[i] > 0)) for i in range(NJ)]


def normalised_rows(J, cols):
    out = []
    for i in range(NJ):
        w = J[i, np.flatnonzero(J[i] > 0)].astype(np.float64)
        out.append(w / w.sum())
    return out


def integer_rows(seed, n, ns):
    """(n, ns + 17, 3) float32 of integers: vertices in [-512, 512], ground truth in [-1000, 1000] mm: every product and every sum of
    the moments is an integer below 2^53"""
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.randint(-512, 513, size=(n, ns, 3)), rng.randint(-1000, 1001, size=(n, NJ, 3))], axis=1).astype(np.float32)


def real_rows(seed, n, ns):
    """(n, ns + 17, 3) float32: vertices of body size in m, pelvis-centred joints of a random simplex regressor in mm with 10 mm noise"""
    rng = np.random.RandomState(seed)
    v = (rng.normal(0, 1, size=(n, ns, 3)) * np.array([0.15, 0.5, 0.1])).astype(np.float32)
    w = rng.dirichlet(np.ones(ns), size=NJ)
    j = np.einsum('je,nec->njc', w, v.astype(np.float64))
    gt = (j - j[:, :1]) * 1000.0 + rng.normal(0, 10.0, size=j.shape)
    return np.concatenate([v, (gt - gt[:, :1]).astype(np.float32)], axis=1)
