"""The exact solve of the regressor fit (`--fit_regressor OUT --fit_from PATH --fit_solve`).

With the meshes fixed, the loss of jrr_jfit_run -- the mean over count * 17 * 3 of (Jn v - Jn_0 v - gt / 1000)^2 -- is a quadratic in
the normalised weights Jn, and relu(J * mask) / rowsum confines each row of Jn to the simplex over its listed entries: a convex QP with
at most 17 * 128 variables, whose data are the second moments of the cache rows (engine.RegressorFit.moments, include/jrr.h
jrr_jfit_moments: one pass over the table, fp64).  This module is the host side, numpy float64, no GPU:

  loss_from_moments   the loss and its gradient per row from M
  solve               the minimiser over the product of the rows' simplices, with the Frank-Wolfe gap as its certificate:
                      gap(x) = sum over rows of (grad_i . x_i - min_e grad_ie)  and  0 <= L(x) - L* <= gap(x)  for a convex loss
  ring_candidates     the rows' lists grown by k rings of mesh edges (`--fit_rings K`): a zero entry of a candidate list can become
                      active, which Adam on relu(J * mask) can never do (relu'(0) = 0)
  solve_command       the command: moments of the training and the held-out rows, the solve, the weights into the state
                      (jrr_jfit_set_entries), scores, checkpoint, OUT/solve.json
  solve_norm          `--fit_solve_loss mpjpe`: the minimiser of the smoothed MPJPE L_delta (include/jrr.h, jrr_jfit_norm_moments) by
                      majorise-minimise -- each pass (the device's, or norm_blocks_reference) gives the objective, its gradient, the gap
                      and a quadratic majoriser, which solve_quadratic_blocks minimises; certificate L(x) - min L <= gap + delta

  price_reference     `--fit_grow R`: the pass of jrr_jfit_price restated -- the gradient of the loss with respect to a weight on EVERY
  price_gradients     vertex of the mesh at the current solution; global_gap: the Frank-Wolfe gap over the whole mesh; grow_select / grow:
  global_gap, grow    column generation -- add the vertices with the most negative reduced cost, drop the zero weights, solve again

The solver is a projected Newton method on the faces of the simplices.  At x the free set is the entries with x > 0 and the entries
at zero whose gradient lies below their row's multiplier grad_i . x_i (they want to enter).  On the free set the sum constraints are
eliminated by a Householder basis per row, and the reduced Hessian, plus a small multiple of the identity (the Gram matrix of
neighbouring vertices is close to singular, and singular when the table has fewer rows than a list has entries), gives the step
direction; the step length is the exact minimiser of the quadratic along it, cut at the first entry that reaches zero, which then
leaves the free set.  Every step lowers the loss; the iteration ends when the gap is at most tol * L(x0).
"""
from __future__ import annotations

import json
import os
from typing import List, Optional, Sequence

import numpy as np

NJ, NV = 17, 6890
ROW_CAP = 128                 # include/jrr.h: JRR_JFIT_ROW_CAP
LAYOUT_VERSION = 1
# what solve.json holds (tests/test_regressor_solve.py checks the schema)
SOLVE_KEYS = ('layout_version', 'source', 'flags', 'rows', 'rings', 'support', 'loss', 'gap', 'tol', 'iterations', 'converged', 'initial',
              'final', 'checkpoint', 'j_regressor_init')
SUPPORT_KEYS = ('before', 'candidates', 'after')
LOSS_KEYS = ('train_before', 'train_after', 'holdout_before', 'holdout_after')


def _lists(lists) -> List[np.ndarray]:
    out = [np.asarray(l, dtype=np.int64).reshape(-1) for l in lists]
    if len(out) != NJ:
        raise ValueError(f'{len(out)} lists: one per joint, {NJ}')
    return out


def _rows(x, lists) -> List[np.ndarray]:
    out = [np.asarray(r, dtype=np.float64).reshape(-1) for r in x]
    if len(out) != NJ or any(r.size != l.size for r, l in zip(out, lists)):
        raise ValueError('x: one row of weights per list, of the list\'s length')
    return out


def loss_from_moments(M, n: int, lists, x):
    """(loss, [gradient of row i]) of the fit's loss at the weights x from the moments M of n cache rows.

    M (W, W), W = ns + 17: jrr_jfit_moments.  lists[i]: the positions in the union (0 .. ns - 1) of row i's entries; x[i]: their
    weights.  The loss is the one jrr_jfit_run states: joints = x_i . v minus joint 0, minus gt / 1000, squared, the mean over
    n * 17 * 3.  A row without entries is left out (the mean still divides by n * 51); an empty pelvis row centres on the origin."""
    M = np.asarray(M, dtype=np.float64)
    W = M.shape[0]
    ns = W - NJ
    lists = _lists(lists)
    x = _rows(x, lists)
    if M.shape != (W, W) or ns < 1 or n < 1:
        raise ValueError(f'moments of shape {M.shape} over {n} rows')
    # residual of joint i on a sample = U[:, i] . (the sample's W points), per axis
    U = np.zeros((W, NJ))
    for i in range(NJ):
        if lists[i].size == 0:
            continue
        if i != 0:
            U[lists[i], i] += x[i]
            if lists[0].size:
                U[lists[0], i] -= x[0]
        U[ns + i, i] -= 1e-3
    MU = M @ U
    c = 1.0 / (float(n) * NJ * 3)
    loss = c * float(np.einsum('wi,wi->', U, MU))
    grads = [np.zeros(l.size) for l in lists]
    for i in range(1, NJ):
        if lists[i].size:
            grads[i] = 2.0 * c * MU[lists[i], i]
            if lists[0].size:
                grads[0] = grads[0] - 2.0 * c * MU[lists[0], i]
    return loss, grads


def fw_gap(x, grads) -> float:
    """the Frank-Wolfe gap of the product of simplices: sum over the rows with entries of grad_i . x_i - min_e grad_ie"""
    return float(sum(float(g @ r) - float(g.min()) for r, g in zip(x, grads) if g.size))


def _hessian(M, n, lists):
    """the Hessian of the loss over the flattened entries, row-major (constant: the loss is a quadratic)"""
    ns = M.shape[0] - NJ
    pos = np.concatenate(lists)
    row = np.concatenate([np.full(l.size, i, dtype=np.int64) for i, l in enumerate(lists)])
    K = np.zeros((NJ, NJ))
    others = [i for i in range(1, NJ) if lists[i].size]
    for i in others:
        K[i, i] = 1.0
        K[i, 0] = K[0, i] = -1.0
    K[0, 0] = float(len(others))
    G = M[:ns, :ns]
    H = (2.0 / (float(n) * NJ * 3)) * G[np.ix_(pos, pos)] * K[np.ix_(row, row)]
    return H, row


def _normalised(xf, row):
    xf = np.maximum(xf, 0.0)
    s = np.bincount(row, weights=xf, minlength=NJ)
    return xf / s[row]


def _newton_direction(H, g, free, row, ridge):
    """the step on the free entries that minimises the quadratic model (Hessian + ridge) subject to every row's entries summing to 0"""
    idx = np.flatnonzero(free)
    p = np.zeros(g.size)
    if idx.size == 0:
        return p
    A = H[np.ix_(idx, idx)].copy()
    b = g[idx].copy()
    r = row[idx]
    starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]])
    ends = np.r_[starts[1:], idx.size]
    vs = []
    for a, e in zip(starts, ends):                     # Q = I - 2 v v^T / v^T v maps ones / sqrt(k) to e_1: columns 2.. span sum = 0
        k = e - a
        v = np.full(k, 1.0 / np.sqrt(k))
        v[0] -= 1.0
        vv = float(v @ v)
        vs.append((v, vv))
        if vv > 0.0:
            A[a:e, :] -= np.outer(v, (2.0 / vv) * (v @ A[a:e, :]))
            A[:, a:e] -= np.outer((2.0 / vv) * (A[:, a:e] @ v), v)
            b[a:e] -= v * ((2.0 / vv) * float(v @ b[a:e]))
    keep = np.ones(idx.size, dtype=bool)
    keep[starts] = False
    if not keep.any():
        return p
    Az = A[np.ix_(keep, keep)]
    Az = 0.5 * (Az + Az.T)
    d = float(np.mean(np.diag(Az)))
    scale = ridge * (d if d > 0.0 else 1.0)
    while True:
        try:
            z = np.linalg.solve(Az + scale * np.eye(Az.shape[0]), -b[keep])
            if np.isfinite(z).all():
                break
        except np.linalg.LinAlgError:
            pass
        scale *= 100.0
    y = np.zeros(idx.size)
    y[keep] = z
    for (a, e), (v, vv) in zip(zip(starts, ends), vs):
        if vv > 0.0:
            y[a:e] -= v * ((2.0 / vv) * float(v @ y[a:e]))
    p[idx] = y
    return p


def solve(M, n: int, lists, x0, tol: float = 1e-6, max_iter: int = 1000, ridge: float = 1e-9) -> dict:
    """minimise loss_from_moments over the product of the rows' simplices, from x0 (rows of non-negative weights, normalised here).

    Returns {'x': rows of weights, 'loss', 'loss0': L(x0), 'gap': the Frank-Wolfe gap at x (0 <= loss - L* <= gap), 'iterations',
    'converged': gap <= tol * L(x0) was reached within max_iter steps}."""
    M = np.asarray(M, dtype=np.float64)
    lists = _lists(lists)
    x0 = _rows(x0, lists)
    sizes = [l.size for l in lists]
    if sum(sizes) == 0:
        raise ValueError('solve: no listed entry')
    cuts = np.cumsum(sizes)[:-1]
    split = lambda xf: np.split(xf, cuts)
    H, row = _hessian(M, n, lists)
    xf = np.concatenate(x0)
    if (xf < 0).any() or (np.bincount(row, weights=xf, minlength=NJ)[np.unique(row)] <= 0).any():
        raise ValueError('solve: x0 needs non-negative rows with a positive sum')
    xf = _normalised(xf, row)
    loss0 = None
    it = 0
    while True:
        loss, grads = loss_from_moments(M, n, lists, split(xf))
        if loss0 is None:
            loss0 = loss
        g = np.concatenate(grads)
        lam = np.bincount(row, weights=xf * g, minlength=NJ)
        gap = fw_gap(split(xf), grads)
        if gap <= tol * loss0 or it >= max_iter:
            break
        it += 1
        free = (xf > 0.0) | (g < lam[row])
        while True:
            p = _newton_direction(H, g, free, row, ridge)
            blocked = free & (xf <= 0.0) & (p < 0.0)
            if not blocked.any():
                break
            free &= ~blocked
        slope = float(g @ p)
        if not slope < 0.0:
            break                                      # no descent direction is left at this precision
        curv = float(p @ (H @ p))
        alpha = -slope / curv if curv > 0.0 else np.inf
        neg = p < 0.0
        room = np.full(xf.size, np.inf)
        room[neg] = xf[neg] / -p[neg]
        amax = float(room.min()) if neg.any() else np.inf
        if not np.isfinite(min(alpha, amax)):
            break
        if amax <= alpha:
            hit = room <= amax
            xf = xf + amax * p
            xf[hit] = 0.0
        else:
            xf = xf + alpha * p
        xf = _normalised(xf, row)
    return {'x': split(xf), 'loss': loss, 'loss0': loss0, 'gap': gap, 'iterations': it, 'converged': bool(gap <= tol * loss0)}


# ---- the MPJPE solve (`--fit_solve_loss mpjpe`; include/jrr.h, jrr_jfit_norm_moments) ---------------------------------------------------
NORM_UNIT, NORM_INV = 0, 1            # include/jrr.h: JRR_JFIT_NORM_*
NORM_KEYS = ('delta_mm', 'objective_mm', 'gap_mm', 'bound_mm', 'passes', 'inner_iterations')
NORM_OBJECTIVE_KEYS = ('start', 'mse', 'final', 'holdout_start', 'holdout_mse', 'holdout_final')
INNER_FRACTION = 0.1                  # a surrogate QP stops at a Frank-Wolfe gap of this fraction of the outer gap it was built at


def norm_block_offsets(counts) -> List[int]:
    """the first double of joint i's block in the output of jrr_jfit_norm_moments, i = 1 .. 16, then the total: entry i - 1 of the list
    (K_i = counts[i] + counts[0], or 0 for an empty row; a block is K_i^2 + K_i + 4 doubles)"""
    counts = [int(c) for c in counts]
    if len(counts) != NJ or min(counts) < 0 or max(counts) > ROW_CAP:
        raise ValueError(f'counts: {NJ} numbers in 0 .. {ROW_CAP}')
    out, o = [], 0
    for i in range(1, NJ):
        K = counts[i] + counts[0] if counts[i] else 0
        out.append(o)
        o += K * K + K + 4
    return out + [o]


def parse_norm_blocks(flat, counts) -> list:
    """the output of jrr_jfit_norm_moments as a list of 17: None for the pelvis, else {'A' (K, K), 'b' (K,), 'rho', 'abs', 'w', 'n',
    'cnt': the joint's own entries -- the first cnt of the K points; the rest are the pelvis row's}"""
    flat = np.asarray(flat, dtype=np.float64).reshape(-1)
    offs = norm_block_offsets(counts)
    if flat.size != offs[-1]:
        raise ValueError(f'{flat.size} doubles for counts that need {offs[-1]}')
    blocks = [None]
    for i in range(1, NJ):
        K = int(counts[i]) + int(counts[0]) if counts[i] else 0
        o = offs[i - 1]
        s = flat[o + K * K + K:o + K * K + K + 4]
        blocks.append({'A': flat[o:o + K * K].reshape(K, K), 'b': flat[o + K * K:o + K * K + K], 'rho': float(s[0]), 'abs': float(s[1]),
                       'w': float(s[2]), 'n': float(s[3]), 'cnt': int(counts[i])})
    return blocks


def norm_blocks_reference(rows, lists, x, mode: int, delta: float, dtype=np.float64) -> list:
    """the pass of jrr_jfit_norm_moments restated in numpy (parse_norm_blocks' form): rows (n, ns + 17, 3) the cache rows as points (the
    union's vertices in m, then the ground truth in mm), lists / x as for loss_from_moments, delta in m.  dtype: the arithmetic."""
    lists = _lists(lists)
    x = _rows(x, lists)
    if mode not in (NORM_UNIT, NORM_INV) or not (np.isfinite(delta) and delta >= 0.0) or (mode == NORM_INV and not delta > 0.0):
        raise ValueError(f'mode {mode} with delta {delta}')
    R = np.asarray(rows).astype(dtype)
    n, W = R.shape[0], R.shape[1]
    ns = W - NJ
    d = dtype(delta)
    thousand = dtype(1000.0)
    blocks = [None]
    P0 = R[:, lists[0]]
    x0 = x[0].astype(dtype)
    for i in range(1, NJ):
        ci = lists[i].size
        if ci == 0:
            blocks.append({'A': np.zeros((0, 0)), 'b': np.zeros(0), 'rho': 0.0, 'abs': 0.0, 'w': 0.0, 'n': 0.0, 'cnt': 0})
            continue
        P = np.concatenate([R[:, lists[i]], P0], axis=1)                      # (n, K, 3)
        wt = np.concatenate([x[i].astype(dtype), -x0])
        r = np.einsum('e,nec->nc', wt, P) - R[:, ns + i] / thousand
        rr = (r * r).sum(1)
        rho = np.sqrt(rr + d * d)
        w = 1.0 / rho if mode == NORM_INV else np.ones(n, dtype=dtype)
        A = np.einsum('n,nac,nbc->ab', w, P, P)
        b = np.einsum('n,nc,nac->a', w, r, P)
        blocks.append({'A': A, 'b': b, 'rho': rho.sum(), 'abs': np.sqrt(rr).sum(), 'w': w.sum(), 'n': float(n), 'cnt': ci})
    return blocks


def norm_objective(blocks, n: int):
    """(L_delta, L): sum rho / (n 17) and sum |r| / (n 17) over the joints' blocks -- 1000 L is the MPJPE in mm of the n rows"""
    c = 1.0 / (float(n) * NJ)
    return c * float(sum(b['rho'] for b in blocks[1:])), c * float(sum(b['abs'] for b in blocks[1:]))


def norm_gradient(blocks, n: int, lists) -> List[np.ndarray]:
    """the gradient of L_delta per row from the b_i of an INV pass: row i takes b_i's first cnt_i elements, the pelvis row minus the sum
    of every joint's second half, all over n 17"""
    lists = _lists(lists)
    c = 1.0 / (float(n) * NJ)
    grads = [np.zeros(l.size) for l in lists]
    for i in range(1, NJ):
        ci = lists[i].size
        if ci == 0:
            continue
        b = np.asarray(blocks[i]['b'], dtype=np.float64)
        if b.size != ci + lists[0].size:
            raise ValueError(f'block {i} has {b.size} points for lists of {ci} + {lists[0].size}')
        grads[i] = c * b[:ci]
        if lists[0].size:
            grads[0] = grads[0] - c * b[ci:]
    return grads


def _block_hessian(blocks, n, lists):
    """the Hessian of the surrogate over the flattened entries: joint x joint A_i[:c, :c], joint x pelvis -A_i[:c, c:], pelvis x pelvis
    the sum of A_i[c:, c:], over n 17"""
    sizes = [l.size for l in lists]
    off = np.concatenate([[0], np.cumsum(sizes)])
    E = int(off[-1])
    H = np.zeros((E, E))
    c0 = sizes[0]
    for i in range(1, NJ):
        ci = sizes[i]
        if ci == 0:
            continue
        A = np.asarray(blocks[i]['A'], dtype=np.float64)
        a, e = int(off[i]), int(off[i]) + ci
        H[a:e, a:e] += A[:ci, :ci]
        if c0:
            H[a:e, :c0] -= A[:ci, ci:]
            H[:c0, a:e] -= A[ci:, :ci]
            H[:c0, :c0] += A[ci:, ci:]
    row = np.concatenate([np.full(s, i, dtype=np.int64) for i, s in enumerate(sizes)])
    return H / (float(n) * NJ), row


def solve_quadratic_blocks(blocks, n: int, lists, x_k, gap_stop: float, max_iter: int = 1000, ridge: float = 1e-9) -> dict:
    """minimise the surrogate Q(x) = const + sum_i [b_i . D_i + 1/2 D_i^T A_i D_i] / (n 17), D_i = (x_i - x_k_i ; -(x_0 - x_k_0)), over the
    product of the rows' simplices from x_k, by the projected Newton method of `solve`; ends at a Frank-Wolfe gap OF THE SURROGATE of
    at most gap_stop.  Every step lowers Q, so the result has Q(x) <= Q(x_k).  Returns {'x', 'gap', 'iterations', 'decrease': Q(x_k) - Q(x)}."""
    lists = _lists(lists)
    x_k = _rows(x_k, lists)
    cuts = np.cumsum([l.size for l in lists])[:-1]
    split = lambda xf: np.split(xf, cuts)
    H, row = _block_hessian(blocks, n, lists)
    g0 = np.concatenate(norm_gradient(blocks, n, lists))
    xk = np.concatenate(x_k)
    xf = xk.copy()
    it = 0
    while True:
        g = g0 + H @ (xf - xk)
        lam = np.bincount(row, weights=xf * g, minlength=NJ)
        gap = fw_gap(split(xf), split(g))
        if gap <= gap_stop or it >= max_iter:
            break
        it += 1
        free = (xf > 0.0) | (g < lam[row])
        while True:
            p = _newton_direction(H, g, free, row, ridge)
            blocked = free & (xf <= 0.0) & (p < 0.0)
            if not blocked.any():
                break
            free &= ~blocked
        slope = float(g @ p)
        if not slope < 0.0:
            break                                      # no descent direction is left at this precision
        curv = float(p @ (H @ p))
        alpha = -slope / curv if curv > 0.0 else np.inf
        neg = p < 0.0
        room = np.full(xf.size, np.inf)
        room[neg] = xf[neg] / -p[neg]
        amax = float(room.min()) if neg.any() else np.inf
        if not np.isfinite(min(alpha, amax)):
            break
        if amax <= alpha:
            hit = room <= amax
            xf = xf + amax * p
            xf[hit] = 0.0
        else:
            xf = xf + alpha * p
        xf = _normalised(xf, row)
    D = xf - xk
    return {'x': split(xf), 'gap': gap, 'iterations': it, 'decrease': -float(g0 @ D + 0.5 * D @ (H @ D))}


def solve_norm(pass_fn, n: int, lists, x0, delta: float, tol: float = 1e-6, max_iter: int = 1000, ridge: float = 1e-9) -> dict:
    """minimise L_delta (include/jrr.h) over the product of the rows' simplices.  pass_fn(x, mode, delta) -> blocks (parse_norm_blocks'
    form) of the n training rows: the device pass, or norm_blocks_reference.  Pass 0 is UNIT at x0: its quadratic is the `--fit_solve`
    problem and its minimiser x_mse the first iterate.  Then INV passes, each followed by the minimisation of its majoriser down to
    INNER_FRACTION of the pass's gap, until gap(L_delta) <= tol * L_delta(x0) or max_iter INV passes.

    Returns {'x', 'x_mse', 'objective': {'start', 'mse', 'final'} (L, m), 'smoothed': the same of L_delta, 'gap' (of L_delta at x),
    'bound': gap + delta >= L(x) - min L, 'passes' (all, the UNIT one included), 'inner_iterations', 'converged',
    'sequence': L_delta at the INV passes -- never rising}."""
    lists = _lists(lists)
    x0 = _rows(x0, lists)
    if not (np.isfinite(delta) and delta > 0.0):
        raise ValueError(f'solve_norm: delta {delta}: finite and positive')
    row = np.concatenate([np.full(l.size, i, dtype=np.int64) for i, l in enumerate(lists)])
    if row.size == 0:
        raise ValueError('solve_norm: no listed entry')
    cuts = np.cumsum([l.size for l in lists])[:-1]
    xf = np.concatenate(x0)
    if (xf < 0).any() or (np.bincount(row, weights=xf, minlength=NJ)[np.unique(row)] <= 0).any():
        raise ValueError('solve_norm: x0 needs non-negative rows with a positive sum')
    x = np.split(_normalised(xf, row), cuts)
    blocks = pass_fn(x, NORM_UNIT, delta)
    Ld0, L0 = norm_objective(blocks, n)
    g = norm_gradient(blocks, n, lists)                             # UNIT: the gradient of the quadratic, not of L_delta
    inner = solve_quadratic_blocks(blocks, n, lists, x, 1e-9 * max(fw_gap(x, g), 0.0), max_iter, ridge)
    x_mse = x = inner['x']
    inner_total, passes, seq = inner['iterations'], 1, []
    mse = None
    while True:
        blocks = pass_fn(x, NORM_INV, delta)
        passes += 1
        Ld, L = norm_objective(blocks, n)
        seq.append(Ld)
        if mse is None:
            mse = (Ld, L)
        g = norm_gradient(blocks, n, lists)
        gap = fw_gap(x, g)
        if gap <= tol * Ld0 or len(seq) >= max_iter:
            break
        inner = solve_quadratic_blocks(blocks, n, lists, x, INNER_FRACTION * gap, max_iter, ridge)
        inner_total += inner['iterations']
        if not inner['decrease'] > 0.0:
            break                                      # the majoriser cannot be lowered at this precision
        x = inner['x']
    return {'x': x, 'x_mse': x_mse, 'objective': {'start': L0, 'mse': mse[1], 'final': L},
            'smoothed': {'start': Ld0, 'mse': mse[0], 'final': Ld}, 'gap': gap, 'bound': gap + float(delta), 'passes': passes,
            'inner_iterations': inner_total, 'converged': bool(gap <= tol * Ld0), 'sequence': seq}


def build_norm_doc(result: dict, delta_mm: float, holdout: Optional[dict]) -> dict:
    """the `norm` key of solve.json from what solve_norm returned; holdout: {'start', 'mse', 'final'} (L, m) of the held-out rows or None"""
    mm = lambda v: None if v is None else 1000.0 * float(v)
    obj = {k: mm(result['objective'][k]) for k in ('start', 'mse', 'final')}
    for k in ('start', 'mse', 'final'):
        obj['holdout_' + k] = mm(holdout[k]) if holdout else None
    return {'delta_mm': float(delta_mm), 'objective_mm': obj, 'gap_mm': mm(result['gap']), 'bound_mm': mm(result['bound']),
            'passes': int(result['passes']), 'inner_iterations': int(result['inner_iterations'])}


def ring_candidates(J_masked, faces, k: int) -> List[np.ndarray]:
    """per row of J_masked (17, V) = J_init * mask: the vertices of its positive entries plus every vertex within k mesh edges of one
    of them, ascending.  faces (F, 3): the triangles of the mesh.  A row above JRR_JFIT_ROW_CAP = 128 candidates raises ValueError."""
    J = np.asarray(J_masked)
    k = int(k)
    if k < 0:
        raise ValueError(f'rings: {k}: 0 or more')
    nv = J.shape[1]
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if k and (f.size == 0 or f.min() < 0 or f.max() >= nv):
        raise ValueError(f'rings: the faces do not index the {nv} vertices of the regressor')
    src = np.concatenate([f[:, 0], f[:, 1], f[:, 2], f[:, 1], f[:, 2], f[:, 0]])
    dst = np.concatenate([f[:, 1], f[:, 2], f[:, 0], f[:, 0], f[:, 1], f[:, 2]])
    out = []
    for i in range(J.shape[0]):
        on = J[i] > 0
        for _ in range(k):
            grown = on.copy()
            grown[dst[on[src]]] = True
            on = grown
        v = np.flatnonzero(on)
        if v.size > ROW_CAP:
            raise ValueError(f'row {i} has {v.size} candidate entries within {k} rings: at most {ROW_CAP}')
        out.append(v)
    return out


def candidate_pattern(cands: Sequence[np.ndarray], nv: int = NV) -> np.ndarray:
    """(17, nv) float32: ones on the candidates -- what the state is prepared from before jrr_jfit_set_entries loads the true values"""
    P = np.zeros((len(cands), nv), dtype=np.float32)
    for i, v in enumerate(cands):
        P[i, v] = 1.0
    return P


# ---- every vertex priced: the certificate over the whole mesh and the growth of the support (`--fit_grow R`; include/jrr.h, jrr_jfit_price) ----
PRICE_MSE, PRICE_NORM = 0, 1          # include/jrr.h: JRR_JFIT_PRICE_*
PRICE_DOUBLES = (NJ - 1) * NV + (NJ - 1) * 4
UNION_CAP = NJ * ROW_CAP              # 2176 vertices in the union of the lists: what the state of the fit holds
GROW_KEYS = ('rounds', 'add', 'max_rounds', 'eligible', 'global_gap', 'global_converged')
GROW_ROUND_KEYS = ('round', 'candidates', 'support', 'loss', 'gap', 'global_gap', 'added', 'dropped', 'min_reduced', 'capped')


def _residuals(verts, gt, cands, x):
    """r (n, 17, 3) float64 in m (row 0 and the empty rows zero), from meshes (n, 6890, 3) and pelvis-centred gt (n, 17, 3) in mm"""
    cands = _lists(cands)
    x = _rows(x, cands)
    V = np.asarray(verts)
    G = np.asarray(gt)
    if V.ndim != 3 or V.shape[1:] != (NV, 3) or G.shape != (V.shape[0], NJ, 3) or V.shape[0] < 1:
        raise ValueError(f'meshes of shape {V.shape} with ground truth of shape {G.shape}')
    for v in cands:
        if v.size > ROW_CAP or (v.size and (v.min() < 0 or v.max() >= NV)) or np.unique(v).size != v.size:
            raise ValueError(f'a list of at most {ROW_CAP} different vertices in 0 .. {NV - 1}')
    if sum(v.size for v in cands) == 0:
        raise ValueError('no listed entry')
    n = V.shape[0]
    q = np.zeros((n, NJ, 3))
    for i in range(NJ):
        if cands[i].size:
            q[:, i] = np.einsum('e,nec->nc', x[i], V[:, cands[i]].astype(np.float64))
    r = np.zeros((n, NJ, 3))
    for i in range(1, NJ):
        if cands[i].size:
            r[:, i] = q[:, i] - q[:, 0] - G[:, i].astype(np.float64) / 1000.0
    return r


def price_reference(verts, gt, cands, x, mode: int, delta: float) -> np.ndarray:
    """the pass of jrr_jfit_price restated in numpy float64, the same output array: S (16, 6890) row-major -- S[i - 1][u] = sum over
    the meshes and axes of a_i,c v[u][c], a_i = r_i (PRICE_MSE) or r_i / rho (PRICE_NORM) -- then per joint i = 1 .. 16 sum r.r, sum rho,
    sum |r| and the samples counted.  verts (n, 6890, 3) m, gt (n, 17, 3) pelvis-centred mm, cands / x: 17 lists of vertices and their
    weights, delta in m."""
    if mode not in (PRICE_MSE, PRICE_NORM) or not (np.isfinite(delta) and delta >= 0.0) or (mode == PRICE_NORM and not delta > 0.0):
        raise ValueError(f'mode {mode} with delta {delta}')
    r = _residuals(verts, gt, cands, x)
    cands = _lists(cands)
    n = r.shape[0]
    rr = (r * r).sum(2)                                            # (n, 17)
    rho = np.sqrt(rr + float(delta) * float(delta))
    a = r / rho[:, :, None] if mode == PRICE_NORM else r
    V2 = np.asarray(verts).astype(np.float64).transpose(0, 2, 1).reshape(3 * n, NV)
    S = a[:, 1:].transpose(1, 0, 2).reshape(NJ - 1, 3 * n) @ V2
    out = np.zeros(PRICE_DOUBLES)
    out[:(NJ - 1) * NV] = S.reshape(-1)
    tail = out[(NJ - 1) * NV:].reshape(NJ - 1, 4)
    for i in range(1, NJ):
        if cands[i].size:
            tail[i - 1] = (rr[:, i].sum(), rho[:, i].sum(), np.sqrt(rr[:, i]).sum(), float(n))
    return out


def price_loss(out, n: int, mode: int) -> float:
    """the loss the prices belong to, from the scalars of the pass: sum r.r / (51 n) (PRICE_MSE) or sum rho / (17 n) (PRICE_NORM: L_delta)"""
    tail = np.asarray(out, dtype=np.float64).reshape(-1)[(NJ - 1) * NV:].reshape(NJ - 1, 4)
    return float(tail[:, 0].sum()) / (float(n) * NJ * 3) if mode == PRICE_MSE else float(tail[:, 1].sum()) / (float(n) * NJ)


def price_gradients(out, n: int, cands, mode: int) -> np.ndarray:
    """g (17, 6890): the gradient of the loss with respect to a weight on vertex u in row i, from the output of the pass over n meshes:
    g_i = 2 S_i / (51 n) (PRICE_MSE) or S_i / (17 n) (PRICE_NORM) for i >= 1, and g_0 = - sum of the g_i of the rows with entries when row
    0 has entries (else zeros).  At listed vertices it is the gradient loss_from_moments / norm_gradient returns."""
    cands = _lists(cands)
    flat = np.asarray(out, dtype=np.float64).reshape(-1)
    if flat.size != PRICE_DOUBLES or n < 1 or mode not in (PRICE_MSE, PRICE_NORM):
        raise ValueError(f'{flat.size} doubles over {n} meshes in mode {mode}')
    c = 2.0 / (float(n) * NJ * 3) if mode == PRICE_MSE else 1.0 / (float(n) * NJ)
    g = np.zeros((NJ, NV))
    for i in range(1, NJ):
        if cands[i].size:
            g[i] = c * flat[(i - 1) * NV:i * NV]
    if cands[0].size:
        g[0] = -g[1:].sum(0)
    return g


def _eligible(eligible, cands) -> np.ndarray:
    E = np.ones((NJ, NV), dtype=bool) if eligible is None else np.asarray(eligible) > 0
    if E.shape != (NJ, NV):
        raise ValueError(f'eligible of shape {E.shape}: ({NJ}, {NV})')
    E = E.copy()
    for i, v in enumerate(cands):
        E[i, v] = True                                             # a listed entry is a vertex of its row whatever the mask says
    return E


def global_gap(g, cands, x, eligible=None):
    """(gap, lambda (17,), min_reduced (17,)): lambda_i = g_i[listed] . x_i, min_reduced_i = min over the eligible u of g_i[u] - lambda_i
    (<= 0), gap = - sum of min_reduced over the rows with entries -- the Frank-Wolfe gap over the product of the simplices on ALL
    eligible vertices, the unlisted ones at weight zero: 0 <= L(x) - min L <= gap.  eligible (17, 6890), > 0 where a vertex may carry
    weight (None: everywhere); rows without entries give zeros."""
    cands = _lists(cands)
    x = _rows(x, cands)
    g = np.asarray(g, dtype=np.float64)
    E = _eligible(eligible, cands)
    lam, low = np.zeros(NJ), np.zeros(NJ)
    for i in range(NJ):
        if cands[i].size:
            lam[i] = float(g[i, cands[i]] @ x[i])
            low[i] = float(g[i][E[i]].min()) - lam[i]
    return float(-low.sum()), lam, low


def grow_select(g, cands, x, eligible, add: int) -> dict:
    """one selection of the column generation.  First every row with entries drops its listed entries whose weight is exactly 0.  Then,
    rows in order 0 .. 16, a row with entries adds up to `add` eligible unlisted vertices with the most negative reduced cost
    g_i[u] - lambda_i, strictly below 0, ties to the lower vertex; never above 128 entries a row or 2176 vertices in the union of the
    lists (`capped`: a cap stopped an addition).  Rows without entries stay empty.  Returns {'cands' (each ascending), 'x' (zeros on the
    new entries), 'added' [17], 'dropped' [17], 'capped'}."""
    cands = _lists(cands)
    x = _rows(x, cands)
    g = np.asarray(g, dtype=np.float64)
    add = int(add)
    if add < 0:
        raise ValueError(f'add {add}: 0 or more')
    E = _eligible(eligible, cands)
    _, lam, _ = global_gap(g, cands, x, E)
    kept, wts, dropped = [], [], [0] * NJ
    for i in range(NJ):
        on = x[i] != 0.0
        dropped[i] = int((~on).sum())
        kept.append(cands[i][on])
        wts.append(x[i][on])
    union = set(np.concatenate(kept).tolist())
    added, capped = [0] * NJ, False
    for i in range(NJ):
        if cands[i].size == 0:
            continue
        red = g[i] - lam[i]
        ok = E[i] & (red < 0.0)
        ok[kept[i]] = False
        pool = np.flatnonzero(ok)
        pool = pool[np.lexsort((pool, red[pool]))]                 # by reduced cost, then by vertex
        new = []
        for u in pool.tolist():
            if len(new) >= add:
                break
            if kept[i].size + len(new) >= ROW_CAP:
                capped = True
                break
            if u not in union:
                if len(union) >= UNION_CAP:                         # (17 rows of at most 128: the row cap always binds first)
                    capped = True
                    continue
                union.add(u)
            new.append(u)
        added[i] = len(new)
        v = np.concatenate([kept[i], np.asarray(new, dtype=np.int64)])
        w = np.concatenate([wts[i], np.zeros(len(new))])
        order = np.argsort(v, kind='stable')
        kept[i], wts[i] = v[order], w[order]
    return {'cands': kept, 'x': wts, 'added': added, 'dropped': dropped, 'capped': capped}


def grow(solve_fn, price_fn, cands, x0, tol: float, rounds: int, add: int, eligible=None, mode: int = PRICE_MSE) -> dict:
    """the column generation: solve -> price -> stop or select -> solve, warm-started at the current weights with zeros on the new entries.
    solve_fn(cands, x_start) returns what `solve` returns ('x', 'loss', 'loss0', 'gap', ...); price_fn(cands, x) returns (the output
    array of the pass, the number of meshes n); `mode` says which loss the prices belong to.  Ends when the global gap is at most
    tol * L(x0) (`global_converged`), when a selection adds nothing, or after `rounds` selections; rounds = 0 solves once and prices once.
    Returns {'cands', 'x', 'rounds': one record (GROW_ROUND_KEYS) per solve, 'global_gap', 'global_converged', 'loss0', 'result': the
    last solve's}."""
    cands = _lists(cands)
    x = _rows(x0, cands)
    rounds, add = int(rounds), int(add)
    if rounds < 0 or add < 1 or not tol > 0.0:
        raise ValueError(f'grow: rounds {rounds} (0 or more), add {add} (1 or more), tol {tol} (positive)')
    records, loss0, k = [], None, 0
    while True:
        res = solve_fn(cands, x)
        x = _rows(res['x'], cands)
        if loss0 is None:
            loss0 = float(res['loss0'])
        out, n = price_fn(cands, x)
        g = price_gradients(out, n, cands, mode)
        gap, _, low = global_gap(g, cands, x, eligible)
        rec = {'round': k, 'candidates': [int(v.size) for v in cands], 'support': [int((r > 0).sum()) for r in x], 'loss': float(res['loss']),
               'gap': float(res['gap']), 'global_gap': gap, 'added': [0] * NJ, 'dropped': [0] * NJ, 'min_reduced': [float(v) for v in low],
               'capped': False}
        records.append(rec)
        converged = bool(gap <= tol * loss0)
        if converged or k >= rounds:
            break
        sel = grow_select(g, cands, x, eligible, add)
        if sum(sel['added']) == 0:
            rec['capped'] = bool(sel['capped'])
            break
        rec.update(added=sel['added'], dropped=sel['dropped'], capped=bool(sel['capped']))
        cands, x = sel['cands'], sel['x']
        k += 1
    return {'cands': cands, 'x': x, 'rounds': records, 'global_gap': gap, 'global_converged': converged, 'loss0': loss0, 'result': res}


def build_grow_doc(result: dict, add: int, max_rounds: int, eligible: int) -> dict:
    """the `grow` key of solve.json from what grow returned (its records may carry the command's scores of the round)"""
    plain = lambda v: v.item() if isinstance(v, np.generic) else v
    rounds = [{k: ([plain(e) for e in v] if isinstance(v, (list, tuple)) else plain(v)) for k, v in r.items()} for r in result['rounds']]
    return {'rounds': rounds, 'add': int(add), 'max_rounds': int(max_rounds), 'eligible': int(eligible),
            'global_gap': float(result['global_gap']), 'global_converged': bool(result['global_converged'])}


def build_doc(source: str, flags: dict, n_train: int, n_holdout: int, rings: int, support_before, candidates, support_after, losses: dict,
              result: dict, tol: float, initial: dict, final: dict, checkpoint: str, j_regressor_init) -> dict:
    """solve.json.  losses: LOSS_KEYS (the held-out ones None without held-out rows); result: what solve returned; initial / final:
    {'train': {mpjpe_mm, pampjpe_mm}, 'holdout': the same or None}"""
    f = lambda v: None if v is None else float(v)
    return {'layout_version': LAYOUT_VERSION, 'source': source, 'flags': flags, 'rows': {'train': int(n_train), 'holdout': int(n_holdout)},
            'rings': int(rings),
            'support': {'before': [int(c) for c in support_before], 'candidates': [int(c) for c in candidates],
                        'after': [int(c) for c in support_after]},
            'loss': {k: f(losses.get(k)) for k in LOSS_KEYS}, 'gap': float(result['gap']), 'tol': float(tol),
            'iterations': int(result['iterations']), 'converged': bool(result['converged']), 'initial': initial, 'final': final,
            'checkpoint': checkpoint, 'j_regressor_init': j_regressor_init}


def solve_command(log=print) -> Optional[dict]:
    """`python main.py --fit_regressor OUT --fit_from PATH --fit_solve [--fit_rings K] [--fit_solve_tol 1e-6] [--fit_solve_iters N]
    [--fit_grow R [--fit_grow_add 8]]`.
    One process: under torchrun rank 0 works and the other ranks return.  Prints one summary line."""
    import torch
    from . import checkpoint, dist as jdist, engine as _engine, regressor_fit as rf, smpl_model, utils
    from .args import args
    ns = args._get()
    rf.check_flags(ns)
    if jdist.env_rank_world()[0] != 0:
        return None
    device = torch.device(ns.device)
    torch.cuda.set_device(device)
    J_np = smpl_model.default_h36m_regressor(ns.j_regressor_init,
                                             allow_default=ns.synthetic or ns.j_regressor_init == 'SPIN/data/J_regressor_h36m.npy')
    J_init = torch.from_numpy(J_np).float().to(device)
    mask = utils.find_j_reg_mask(J_init)
    mask_np = mask.cpu().numpy()
    Jm = J_np * mask_np
    rings = int(ns.fit_rings)
    if rings > 0:
        faces = smpl_model.load_smpl_model(ns.smpl_dir, ns.synthetic or ns.smpl_dir == 'SPIN/data/smpl').get('faces')
        if faces is None:
            raise ValueError('--fit_rings: the body model has no faces')
        cands = ring_candidates(Jm, faces, rings)
    else:
        rf.support_lists(J_np, mask_np)                            # a row above 128 entries is refused here, before any table is read
        cands = ring_candidates(Jm, np.zeros((0, 3), dtype=np.int64), 0)
    empty = [i for i, v in enumerate(cands) if v.size == 0]
    if empty:
        log(f'--fit_solve: rows {empty} of --j_regressor_init have no positive entry: they have no parameters, stay as they are and are '
            f'left out of the loss; their joints evaluate as NaN')
    source = rf._VerticesSource(ns) if rf.is_vertices_dir(ns.fit_from) else rf._RefinedSource(ns, device)
    rows = np.asarray(source.rows)
    held = rf.holdout_split(rows.size, ns.fit_holdout, source.paths)
    order = np.concatenate([rows[~held], rows[held]])
    n_train, n_hold = int((~held).sum()), int(held.sum())
    if n_train == 0:
        raise ValueError(f'--fit_regressor: no training row ({rows.size} rows, {n_hold} held out)')
    # the state: prepared from the candidate pattern, then given the true initial values (zeros on the new candidates)
    if rings > 0:
        jf = _engine.RegressorFit(torch.from_numpy(candidate_pattern(cands)).to(device), mask, order.size)
        jf.J_init = J_init.clone()                                 # what dense() fills the unlisted elements with
        jf.set_entries(J_init)
    else:
        jf = _engine.RegressorFit(J_init, mask, order.size)
    rf.fill_cache(jf, source, order, int(ns.batch_size), device)
    before = rf._score_doc(rf._scores(jf, n_train, n_hold).cpu().numpy())
    cols = np.unique(np.concatenate(cands))
    assert cols.size == jf.ns and [v.size for v in cands] == jf.counts
    lists = [np.searchsorted(cols, v) for v in cands]
    x0 = []
    for i, v in enumerate(cands):
        r = np.maximum(Jm[i, v].astype(np.float64), 0.0)
        x0.append(r / r.sum() if v.size else r)
    tol = float(ns.fit_solve_tol)
    mpjpe = getattr(ns, 'fit_solve_loss', 'mse') == 'mpjpe'
    delta = float(ns.fit_solve_delta_mm) / 1000.0

    def run_solve(jf, lists, x_start):
        """the solve on a filled state: (result, moments of the training rows, of the held-out rows, the `norm` document or None)"""
        M_train = jf.moments(0, n_train).cpu().numpy()
        M_hold = jf.moments(n_train, n_hold).cpu().numpy() if n_hold else None
        jf.info()                                                  # raises if the device refused a call
        if not mpjpe:
            return solve(M_train, n_train, lists, x_start, tol=tol, max_iter=int(ns.fit_solve_iters)), M_train, M_hold, None
        # the MPJPE itself: reweighted moment passes on the device, the quadratics on the host; the MSE loss block below then says
        # what the switch costs in MSE; `gap` is the gap of the smoothed MPJPE in m, `iterations` the Newton steps of all quadratics
        blocks_of = lambda x, mode, d, a, c: parse_norm_blocks(jf.norm_moments(x, mode, d, a, c).cpu().numpy(), jf.counts)
        nres = solve_norm(lambda x, mode, d: blocks_of(x, mode, d, 0, n_train), n_train, lists, x_start, delta, tol=tol,
                          max_iter=int(ns.fit_solve_iters))
        held_obj = None
        if n_hold:
            held_obj = {k: norm_objective(blocks_of(xs, NORM_INV, delta, n_train, n_hold), n_hold)[1]
                        for k, xs in (('start', x_start), ('mse', nres['x_mse']), ('final', nres['x']))}
        jf.info()
        res = {'x': nres['x'], 'loss0': loss_from_moments(M_train, n_train, lists, x_start)[0],
               'loss': loss_from_moments(M_train, n_train, lists, nres['x'])[0], 'gap': nres['gap'], 'iterations': nres['inner_iterations'],
               'converged': nres['converged'], 'smoothed': nres['smoothed']}
        return res, M_train, M_hold, build_norm_doc(nres, float(ns.fit_solve_delta_mm), held_obj)

    res, M_train, M_hold, norm_doc = run_solve(jf, lists, x0)
    losses = {'train_before': res['loss0'], 'train_after': res['loss'], 'holdout_before': None, 'holdout_after': None}
    if n_hold:
        losses['holdout_before'] = loss_from_moments(M_hold, n_hold, lists, x0)[0]
    grow_doc, J_fill = None, J_np
    if getattr(ns, 'fit_grow', None) is not None:
        # every vertex priced at the solution; the support grows where the reduced costs are negative and the solve runs again on a
        # state prepared from the new lists: two passes over the source per round (the cache fill and the prices)
        eligible = mask_np > 0
        J_base = J_np.copy()                                       # what the unlisted elements of a grown row hold: zeros
        for i, v in enumerate(cands):
            J_base[i, v] = 0.0
        cur = {'jf': jf, 'lists': lists, 'M_hold': M_hold, 'first': res}
        extras = []

        def dense_of(c, xs):
            Jd = J_base.copy()
            for i, v in enumerate(c):
                Jd[i, v] = np.asarray(xs[i], dtype=np.float32)
            return Jd

        def solve_fn(c, x_start):
            if cur['first'] is not None:                           # round 0 is the solve above
                r, cur['first'] = cur['first'], None
            else:
                f = _engine.RegressorFit(torch.from_numpy(candidate_pattern(c)).to(device), mask, order.size)
                f.J_init = torch.from_numpy(J_base).to(device)
                f.set_entries(torch.from_numpy(dense_of(c, x_start)).to(device))
                rf.fill_cache(f, source, order, int(ns.batch_size), device)
                cols_ = np.unique(np.concatenate(c))
                assert cols_.size == f.ns and [v.size for v in c] == f.counts
                ls = [np.searchsorted(cols_, v) for v in c]
                r, _, mh, nd = run_solve(f, ls, x_start)
                cur.update(jf=f, lists=ls, M_hold=mh, norm=nd)
            f = cur['jf']
            f.set_entries(torch.from_numpy(dense_of(c, r['x'])).to(device))
            extra = dict(rf._score_doc(rf._scores(f, n_train, n_hold).cpu().numpy()), holdout_loss=None)
            if n_hold:
                extra['holdout_loss'] = float(loss_from_moments(cur['M_hold'], n_hold, cur['lists'], r['x'])[0])
            extras.append(extra)
            if mpjpe:                                              # the prices are those of the smoothed MPJPE: so are loss and gap of a round
                return dict(r, mse=r['loss'], loss=r['smoothed']['final'], loss0=r['smoothed']['start'])
            return r

        def price_fn(c, xs):
            out = None
            with torch.no_grad():
                for a in range(0, n_train, int(ns.batch_size)):
                    verts, gt = source.chunk(order[a:min(a + int(ns.batch_size), n_train)], device)
                    out = _engine.price_vertices(verts, gt, c, None, xs, PRICE_NORM if mpjpe else PRICE_MSE, delta if mpjpe else 0.0,
                                                 out=out, accumulate=out is not None)
            return out.cpu().numpy(), n_train

        gres = grow(solve_fn, price_fn, cands, x0, tol, int(ns.fit_grow), int(ns.fit_grow_add), eligible,
                    PRICE_NORM if mpjpe else PRICE_MSE)
        for rec, extra in zip(gres['rounds'], extras):
            rec.update(extra)
        grow_doc = build_grow_doc(gres, int(ns.fit_grow_add), int(ns.fit_grow), int(eligible.sum()))
        last = gres['result']
        res = dict(last, loss0=res['loss0'], loss=last.get('mse', last['loss']))
        cands, jf, lists, M_hold = gres['cands'], cur['jf'], cur['lists'], cur['M_hold']
        norm_doc = cur.get('norm', norm_doc)
        losses['train_after'] = res['loss']
        J_fill = J_base
    if n_hold:
        losses['holdout_after'] = loss_from_moments(M_hold, n_hold, lists, res['x'])[0]
    # the normalised weights are the raw values; zeros stay zeros
    J_new = J_fill.copy()
    for i, v in enumerate(cands):
        J_new[i, v] = res['x'][i].astype(np.float32)
    jf.set_entries(torch.from_numpy(J_new).to(device))
    after = rf._score_doc(rf._scores(jf, n_train, n_hold).cpu().numpy())
    jf.info()
    J, _, _ = jf.dense()
    path = ns.save_j_regressor or os.path.join(ns.fit_regressor, rf.CHECKPOINT_NAME)
    os.makedirs(ns.fit_regressor, exist_ok=True)
    checkpoint.save_j_regressor(J, path)
    doc = build_doc(source.kind, rf.flags_doc(ns), n_train, n_hold, rings, rf.support_counts(J_np, mask_np), [v.size for v in cands],
                    rf.support_counts(J.cpu().numpy(), mask_np), losses, res, tol, before, after, path, ns.j_regressor_init)
    if norm_doc is not None:
        doc['norm'] = norm_doc
    if grow_doc is not None:
        doc['grow'] = grow_doc
    with open(os.path.join(ns.fit_regressor, 'solve.json'), 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True, default=str)
    fmt = lambda d, k: '-' if d is None or d[k] is None else format(d[k], '.4f')
    extra = ''
    if norm_doc is not None:
        o = norm_doc['objective_mm']
        extra = (f', objective MPJPE in {norm_doc["passes"]} passes: {o["start"]:.4f} mm at the start, {o["mse"]:.4f} mm at the MSE optimum, '
                 f'{o["final"]:.4f} mm at the end, at most {norm_doc["bound_mm"]:.3e} mm above the optimum (delta {norm_doc["delta_mm"]:g} mm)')
    if grow_doc is not None:
        extra += (f', over the whole mesh ({grow_doc["eligible"]} eligible entries): global gap {grow_doc["global_gap"]:.3e} '
                  f'({"converged" if grow_doc["global_converged"] else "NOT converged"}) after {len(grow_doc["rounds"]) - 1} of at most '
                  f'{grow_doc["max_rounds"]} rounds of up to {grow_doc["add"]} vertices a row')
    log(f'solved the regressor on {n_train} rows ({n_hold} held out, {jf.entries} entries on {jf.ns} vertices, {rings} rings) in '
        f'{res["iterations"]} steps: loss {res["loss0"]:.6e} -> {res["loss"]:.6e}, gap {res["gap"]:.3e} '
        f'({"converged" if res["converged"] else "NOT converged"} at tol {tol:g}), support {sum(doc["support"]["before"])} -> '
        f'{sum(doc["support"]["after"])}, MPJPE {fmt(before["train"], "mpjpe_mm")} -> {fmt(after["train"], "mpjpe_mm")} (held out '
        f'{fmt(before["holdout"], "mpjpe_mm")} -> {fmt(after["holdout"], "mpjpe_mm")}), PAMPJPE {fmt(before["train"], "pampjpe_mm")} -> '
        f'{fmt(after["train"], "pampjpe_mm")} (held out {fmt(before["holdout"], "pampjpe_mm")} -> {fmt(after["holdout"], "pampjpe_mm")}){extra}; {path}')
    return doc
