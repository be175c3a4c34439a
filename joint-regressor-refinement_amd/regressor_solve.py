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
    """`python main.py --fit_regressor OUT --fit_from PATH --fit_solve [--fit_rings K] [--fit_solve_tol 1e-6] [--fit_solve_iters N]`.
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
    M_train = jf.moments(0, n_train).cpu().numpy()
    M_hold = jf.moments(n_train, n_hold).cpu().numpy() if n_hold else None
    jf.info()                                                      # raises if the device refused a call
    cols = np.unique(np.concatenate(cands))
    assert cols.size == jf.ns and [v.size for v in cands] == jf.counts
    lists = [np.searchsorted(cols, v) for v in cands]
    x0 = []
    for i, v in enumerate(cands):
        r = np.maximum(Jm[i, v].astype(np.float64), 0.0)
        x0.append(r / r.sum() if v.size else r)
    tol = float(ns.fit_solve_tol)
    res = solve(M_train, n_train, lists, x0, tol=tol, max_iter=int(ns.fit_solve_iters))
    losses = {'train_before': res['loss0'], 'train_after': res['loss'], 'holdout_before': None, 'holdout_after': None}
    if n_hold:
        losses['holdout_before'] = loss_from_moments(M_hold, n_hold, lists, x0)[0]
        losses['holdout_after'] = loss_from_moments(M_hold, n_hold, lists, res['x'])[0]
    # the normalised weights are the raw values; zeros stay zeros
    J_new = J_np.copy()
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
    with open(os.path.join(ns.fit_regressor, 'solve.json'), 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True, default=str)
    fmt = lambda d, k: '-' if d is None or d[k] is None else format(d[k], '.4f')
    log(f'solved the regressor on {n_train} rows ({n_hold} held out, {jf.entries} entries on {jf.ns} vertices, {rings} rings) in '
        f'{res["iterations"]} steps: loss {res["loss0"]:.6e} -> {res["loss"]:.6e}, gap {res["gap"]:.3e} '
        f'({"converged" if res["converged"] else "NOT converged"} at tol {tol:g}), support {sum(doc["support"]["before"])} -> '
        f'{sum(doc["support"]["after"])}, MPJPE {fmt(before["train"], "mpjpe_mm")} -> {fmt(after["train"], "mpjpe_mm")} (held out '
        f'{fmt(before["holdout"], "mpjpe_mm")} -> {fmt(after["holdout"], "mpjpe_mm")}), PAMPJPE {fmt(before["train"], "pampjpe_mm")} -> '
        f'{fmt(after["train"], "pampjpe_mm")} (held out {fmt(before["holdout"], "pampjpe_mm")} -> {fmt(after["holdout"], "pampjpe_mm")}); {path}')
    return doc
