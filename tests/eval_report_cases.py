"""Host restatement and seeded inputs of the evaluation report (tests/test_eval_report.py, tests/test_gpu_eval_report.py,
tests/golden/make_golden_eval.py).

Written from the reference's lines -- evaluate (/root/reference/scripts/utils.py:117-145), batch_compute_similarity_transform_torch
(scripts/eval_utils.py:7-58), find_joints (scripts/utils.py:87-98) -- and from the table layout of include/jrr.h (JRR_EVAL_ACC_*).
Large inputs are regenerated from numpy.random.RandomState seeds here, never stored.

Bounds: `bound(d) = 3 d + 1e-7` with d the distance of the reference's float32 evaluation from the float64 one ON THE TEST'S OWN
INPUTS (the project's margin: DESIGN.md sections 3a, 3c, 3d)."""
import numpy as np
import torch

F = np.float32
NJ, NV = 17, 6890
ROW, TRAILER = 338, 2
COUNT, BAD, SUM, SUM_PA, HIST, HIST_PA, BINS = 0, 1, 2, 19, 36, 187, 151
N_MIRRORED = 10


def bound(d: float) -> float:
    return 3.0 * float(d) + 1e-7


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------
def _rodrigues(aa: np.ndarray) -> np.ndarray:
    th = np.linalg.norm(aa, axis=1, keepdims=True)
    k = aa / np.maximum(th, 1e-12)
    K = np.zeros((aa.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    th = th[:, :, None]
    return np.eye(3)[None] + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def pose_cases(B: int, seed: int):
    """(pred (B,17,3) m, target_mm (B,17,3)) float32, as tests/test_gpu_parity.py:314-319 builds them: the target is the prediction
    rotated (large angles), scaled 1.3, shifted, with 20 mm noise; the first min(B, 10) targets are mirrored, so the det-sign branch
    of the Procrustes solution runs"""
    rs = np.random.RandomState(seed)
    pred = rs.randn(B, NJ, 3) * 0.3
    R = _rodrigues(rs.randn(B, 3) * 2.0)
    tgt = (np.einsum('brc,bic->bir', R, pred) * 1.3 + 0.2 + rs.randn(B, NJ, 3) * 0.02) * 1000
    tgt[:N_MIRRORED, :, 0] *= -1
    return pred.astype(F), tgt.astype(F)


# ---- seeded inputs: poses shaped like bodies, and the degenerate shapes behind them ----------------------------------------------
BODY = (0.15, 0.5, 0.05)                               # extents of a standing body in metres
# name -> (seed, cap in metres on the reference's own float32-to-float64 distance of the PA error: a condition on the INPUTS,
# asserted by tests/test_eval_report.py -- if a seed breaks it, another seed is picked, never a wider cap)
FAMILIES = {
    'body': (1, 5e-6), 'thin_0.01': (2, 5e-6), 'thin_0.002': (3, 5e-6), 'flat_target': (4, 5e-6), 'flat_pred': (5, 5e-6),
    'flat_both_mirrored': (6, 5e-6), 'near_line': (7, 1e-5), 'collinear_pred': (8, 5e-6), 'collinear_target': (9, 5e-6),
    'scaled_1e-3': (1, 5e-6), 'scaled_50': (1, 5e-6), 'identical': (1, 5e-6), 'constant_target': (10, 5e-6),
    'constant_pred': (11, 5e-6),
}
ALL_NAN_PA = ('constant_pred',)                        # the reference's 0/0: all 17 PA values NaN, the plain errors finite
G11_FAMILIES = ('body', 'thin_0.002', 'flat_target', 'flat_both_mirrored', 'collinear_pred', 'constant_target')
G11_POSES = 8                                          # per family in tests/golden/g11_eval_degenerate.npz


def family_cases(name: str, B: int, seed=None):
    """(pred (B,17,3) m, target_mm (B,17,3)) float32 of one family of FAMILIES.  A cloud is shaped in its own axes (`extents`), a
    target is made there as 1.3 x the cloud + noise, coordinates are zeroed where the family says "exactly", every second target is
    mirrored where it says so; then pred gets a random rigid rotation (no family is axis-aligned) and the target the same one
    followed by a second large one and a shift of 0.2 m.  "Exactly" planar or collinear means: before the rotations; afterwards
    to the rounding of float32."""
    seed = FAMILIES[name][0] if seed is None else seed
    rs = np.random.RandomState(seed)
    extents, noise, zero_pred, zero_tgt, mirrored = BODY, 0.02, (), (), False
    if name in ('body', 'scaled_1e-3', 'scaled_50', 'identical', 'constant_target', 'constant_pred'):
        mirrored = name != 'identical'
    elif name == 'thin_0.01':
        extents, noise = (0.15, 0.5, 0.01), 0.005
    elif name == 'thin_0.002':
        extents, noise = (0.15, 0.5, 0.002), 0.001
    elif name == 'flat_target':
        zero_tgt = (2,)
    elif name == 'flat_pred':
        zero_pred = (2,)
    elif name == 'flat_both_mirrored':
        zero_pred, zero_tgt, mirrored = (2,), (2,), True
    elif name == 'near_line':
        extents, noise = (0.01, 0.5, 0.01), 0.005
    elif name == 'collinear_pred':
        zero_pred = (0, 2)
    elif name == 'collinear_target':
        zero_tgt = (0, 2)
    else:
        raise KeyError(name)
    base = rs.randn(B, NJ, 3) * np.asarray(extents)
    for c in zero_pred:
        base[:, :, c] = 0
    tb = 1.3 * base + rs.randn(B, NJ, 3) * noise
    for c in zero_tgt:
        tb[:, :, c] = 0
    if mirrored:
        tb[::2, :, 0] *= -1
    R0, R1 = _rodrigues(rs.randn(B, 3) * 2.0), _rodrigues(rs.randn(B, 3) * 2.0)
    pred = np.einsum('brc,bic->bir', R0, base)
    tgt = (np.einsum('brc,bic->bir', R1 @ R0, tb) + 0.2) * 1000
    if name == 'scaled_1e-3':
        pred = pred * 1e-3
    elif name == 'scaled_50':
        pred = pred * 50
    elif name == 'identical':
        return pred.astype(F), (pred.astype(F) * F(1000)).astype(F)
    elif name == 'constant_target':
        tgt[:] = tgt[:, [3], :]
    elif name == 'constant_pred':
        pred[:] = pred[:, [3], :]
    return pred.astype(F), tgt.astype(F)


def mixed_cases(B: int, names=None):
    """(pred, target_mm, family index (B,), rows within the family's own batch (B,)): pose b is pose b // n of family b mod n, so
    every 64-pose wave holds every rank"""
    names = list(FAMILIES) if names is None else list(names)
    n = len(names)
    per = {k: family_cases(k, (B + n - 1) // n) for k in names}
    fam, row = np.arange(B) % n, np.arange(B) // n
    pred = np.stack([per[names[f]][0][r] for f, r in zip(fam, row)])
    tgt = np.stack([per[names[f]][1][r] for f, r in zip(fam, row)])
    return pred, tgt, fam, row


def mesh_cases(n: int, seed: int) -> np.ndarray:
    """(n,6890,3) float32 vertices: a body-sized cloud, not centred"""
    rs = np.random.RandomState(seed)
    return (rs.randn(n, NV, 3) * 0.4 + rs.randn(n, 1, 3) * 0.5).astype(F)


def dense_regressor(seed: int, zero_row=None) -> np.ndarray:
    """(17,6890) float32, every entry positive (all 117 130); zero_row: that row set to zero"""
    J = (np.random.RandomState(seed).rand(NJ, NV) + 0.01).astype(F)
    if zero_row is not None:
        J[zero_row] = 0
    return J


# ---- restatement: evaluate without the means --------------------------------------------------------------------------------
def procrustes(S1: torch.Tensor, S2: torch.Tensor) -> torch.Tensor:
    """scripts/eval_utils.py:7-58 for (B,N,3) inputs, in the inputs' dtype"""
    S1, S2 = S1.permute(0, 2, 1), S2.permute(0, 2, 1)
    mu1, mu2 = S1.mean(dim=-1, keepdim=True), S2.mean(dim=-1, keepdim=True)
    X1, X2 = S1 - mu1, S2 - mu2
    var1 = torch.sum(X1 ** 2, dim=1).sum(dim=1)
    K = X1.bmm(X2.permute(0, 2, 1))
    U, s, V = torch.svd(K)
    Z = torch.eye(3, dtype=S1.dtype).unsqueeze(0).repeat(U.shape[0], 1, 1)
    Z[:, -1, -1] *= torch.sign(torch.det(U.bmm(V.permute(0, 2, 1))))
    R = V.bmm(Z.bmm(U.permute(0, 2, 1)))
    scale = torch.stack([torch.trace(x) for x in R.bmm(K)]) / var1
    t = mu2 - scale[:, None, None] * R.bmm(mu1)
    return (scale[:, None, None] * R.bmm(S1) + t).permute(0, 2, 1)


def evaluate_joints(pred, target_mm, dtype=torch.float32):
    """(s1hat (B,17,3), err_j (B,17), err_pa_j (B,17)) in metres: scripts/utils.py:121-138 up to, and without, `.mean(dim=-1)`"""
    p = torch.as_tensor(np.asarray(pred)).to(dtype)
    t = torch.as_tensor(np.asarray(target_mm)).to(dtype) / 1000
    p = p - p[:, [0], :]
    t = t - t[:, [0], :]
    err_j = torch.sqrt(((p - t) ** 2).sum(dim=-1))
    s1hat = procrustes(p, t)
    err_pa_j = torch.sqrt(((s1hat - t) ** 2).sum(dim=-1))
    return s1hat.numpy(), err_j.numpy(), err_pa_j.numpy()


def pose_means(err_j: np.ndarray, err_pa_j: np.ndarray):
    """the per-pose means as k_evaluate forms them, in float32: joint 16 down to 0 for the plain error, 0 up to 16 for the aligned
    one, then / 17"""
    e = np.zeros(err_j.shape[0], dtype=F)
    for i in range(NJ - 1, -1, -1):
        e = (e + err_j[:, i].astype(F)).astype(F)
    pa = np.zeros(err_j.shape[0], dtype=F)
    for i in range(NJ):
        pa = (pa + err_pa_j[:, i].astype(F)).astype(F)
    return (e / F(NJ)).astype(F), (pa / F(NJ)).astype(F)


# ---- restatement: the statements of csrc/evalk.h in float32, operation by operation -----------------------------------------------
def _orthogonal_unit(a):
    """a unit vector orthogonal to a ((B,3) unit vectors): a x (the coordinate axis of a's smallest component), normalised"""
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    o = np.zeros_like(x)
    first, second = (ax <= ay) & (ax <= az), ay <= az
    w = np.stack([np.where(first, o, np.where(second, -z, y)), np.where(first, z, np.where(second, o, -x)),
                  np.where(first, -y, np.where(second, x, o))], 1)
    return _unit(w)


def _unit(w):
    n = np.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2])
    return w / n[:, None]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def kernel_rotation(K):
    """R (B,3,3) float32 of evalk.h for K (B,3,3) float32: one-sided Jacobi on K's columns (6 sweeps over the pairs (0,1), (0,2),
    (1,2)), the static sort, then the rank-2 / rank-1 / rank-0 completion.  Every array stays float32; every lane-wise branch of
    the kernel is a np.where here."""
    G, V = K.astype(F).copy(), np.broadcast_to(np.eye(3, dtype=F), K.shape).copy()
    with np.errstate(all='ignore'):
        for _ in range(6):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                al = G[:, 0, p] * G[:, 0, p] + G[:, 1, p] * G[:, 1, p] + G[:, 2, p] * G[:, 2, p]
                be = G[:, 0, q] * G[:, 0, q] + G[:, 1, q] * G[:, 1, q] + G[:, 2, q] * G[:, 2, q]
                ga = G[:, 0, p] * G[:, 0, q] + G[:, 1, p] * G[:, 1, q] + G[:, 2, p] * G[:, 2, q]
                rot = np.abs(ga) > F(1e-9) * (np.sqrt(al) * np.sqrt(be))
                zeta = (be - al) / (F(2) * ga)
                t = np.copysign(F(1), zeta) / (np.abs(zeta) + np.sqrt(zeta * zeta + F(1)))
                c = F(1) / np.sqrt(t * t + F(1))
                s = t * c
                for M in (G, V):
                    for r in range(3):
                        mp, mq = M[:, r, p].copy(), M[:, r, q].copy()
                        M[:, r, p] = np.where(rot, c * mp - s * mq, mp)
                        M[:, r, q] = np.where(rot, s * mp + c * mq, mq)
        sig = [np.sqrt(G[:, 0, k] * G[:, 0, k] + G[:, 1, k] * G[:, 1, k] + G[:, 2, k] * G[:, 2, k]) for k in range(3)]
        for a, c in ((0, 1), (1, 2), (0, 1)):                     # descending, the kernel's compare-exchange network
            sw = sig[a] < sig[c]
            sig[a], sig[c] = np.where(sw, sig[c], sig[a]), np.where(sw, sig[a], sig[c])
            for M in (G, V):
                ma, mc = M[:, :, a].copy(), M[:, :, c].copy()
                M[:, :, a], M[:, :, c] = np.where(sw[:, None], mc, ma), np.where(sw[:, None], ma, mc)
        u1, v1 = G[:, :, 0] / sig[0][:, None], V[:, :, 0]
        rank1 = (sig[1] <= F(1e-6) * sig[0])[:, None]
        u2 = np.where(rank1, _orthogonal_unit(u1), G[:, :, 1] / sig[1][:, None])
        v2 = np.where(rank1, _orthogonal_unit(v1), V[:, :, 1])
        u3 = _unit(_cross(u1, u2))
        u2 = _cross(u3, u1)
        v3 = _unit(_cross(v1, v2))
        R = np.empty_like(G)
        for r in range(3):
            for c in range(3):
                R[:, r, c] = v1[:, r] * u1[:, c] + v2[:, r] * u2[:, c] + v3[:, r] * u3[:, c]
        rank0 = ~(sig[0] > F(0))                                   # K = 0, and a NaN pose (which is NaN whatever R is)
        return np.where(rank0[:, None, None], np.eye(3, dtype=F)[None], R).astype(F)


def kernel_evaluate_joints(pred, target_mm):
    """(err_j (B,17), err_pa_j (B,17)) float32 in metres: csrc/evalk.h restated in numpy float32, in the kernel's order of operations
    (the compiler's fused multiply-adds are the one thing not restated, so the kernels are compared with this in print only)"""
    P, Q = np.asarray(pred, dtype=F).copy(), (np.asarray(target_mm, dtype=F) / F(1000)).astype(F)
    B = P.shape[0]
    err, err_pa = np.zeros((B, NJ), dtype=F), np.zeros((B, NJ), dtype=F)
    with np.errstate(all='ignore'):
        for i in range(NJ - 1, -1, -1):
            d2 = np.zeros(B, dtype=F)
            for c in range(3):
                P[:, i, c] = P[:, i, c] - P[:, 0, c]
                Q[:, i, c] = Q[:, i, c] - Q[:, 0, c]
                d = P[:, i, c] - Q[:, i, c]
                d2 = d2 + d * d
            err[:, i] = np.sqrt(d2)
        mu1, mu2 = np.zeros((B, 3), dtype=F), np.zeros((B, 3), dtype=F)
        for i in range(NJ):
            mu1, mu2 = mu1 + P[:, i], mu2 + Q[:, i]
        mu1, mu2 = mu1 / F(NJ), mu2 / F(NJ)
        K, var1 = np.zeros((B, 3, 3), dtype=F), np.zeros(B, dtype=F)
        for i in range(NJ):
            x1, x2 = P[:, i] - mu1, Q[:, i] - mu2
            for c in range(3):
                var1 = var1 + x1[:, c] * x1[:, c]
            for r in range(3):
                for c in range(3):
                    K[:, r, c] = K[:, r, c] + x1[:, r] * x2[:, c]
        R = kernel_rotation(K)
        tr = np.zeros(B, dtype=F)
        for r in range(3):
            tr = tr + (R[:, r, 0] * K[:, 0, r] + R[:, r, 1] * K[:, 1, r] + R[:, r, 2] * K[:, 2, r])
        scale = tr / var1
        t = np.stack([mu2[:, r] - scale * (R[:, r, 0] * mu1[:, 0] + R[:, r, 1] * mu1[:, 1] + R[:, r, 2] * mu1[:, 2]) for r in range(3)], 1)
        for i in range(NJ):
            d2 = np.zeros(B, dtype=F)
            for r in range(3):
                h = scale * (R[:, r, 0] * P[:, i, 0] + R[:, r, 1] * P[:, i, 1] + R[:, r, 2] * P[:, i, 2]) + t[:, r]
                d = h - Q[:, i, r]
                d2 = d2 + d * d
            err_pa[:, i] = np.sqrt(d2)
    assert err.dtype == F and err_pa.dtype == F and R.dtype == F and scale.dtype == F
    return err, err_pa


# ---- restatement: joints of given vertices ----------------------------------------------------------------------------------
def regress(verts, J, mask=None, dtype=torch.float32) -> np.ndarray:
    """scripts/utils.py:87-98 on given vertices: J*mask, ReLU, each row divided by its sum, the batched product.  (B,17,3)"""
    J = torch.as_tensor(np.asarray(J)).to(dtype)
    v = torch.as_tensor(np.asarray(verts)).to(dtype)
    if mask is not None:
        J = J * torch.as_tensor(np.asarray(mask)).to(dtype)
    Jn = torch.relu(J)
    Jn = Jn / torch.sum(Jn, dim=1).unsqueeze(1).expand(Jn.shape)
    return torch.matmul(Jn[None].expand(v.shape[0], -1, -1), v).numpy()


# ---- restatement: the accumulator -------------------------------------------------------------------------------------------
def accumulate(err_j, err_pa_j, group, n_groups: int, table=None) -> np.ndarray:
    """ADD to `table` (int64, n_groups * 338 + 2; None = zeros) what jrr_eval_accumulate adds, in exact integers"""
    table = np.zeros(n_groups * ROW + TRAILER, dtype=np.int64) if table is None else table.copy()
    e0, e1 = np.asarray(err_j, dtype=F), np.asarray(err_pa_j, dtype=F)
    for b, g in enumerate(np.asarray(group).tolist()):
        if g < 0:
            table[n_groups * ROW + 0] += 1
            continue
        if g >= n_groups:
            table[n_groups * ROW + 1] += 1
            continue
        row = table[g * ROW:(g + 1) * ROW]
        with np.errstate(invalid='ignore'):
            good = bool(np.all(e0[b] < F(1.0e3)) and np.all(e1[b] < F(1.0e3)))
        if not good:
            row[BAD] += 1
            continue
        row[COUNT] += 1
        for e, s0, h0 in ((e0[b], SUM, HIST), (e1[b], SUM_PA, HIST_PA)):
            fixed = np.rint((e * F(16777216.0)).astype(F).astype(np.float64)).astype(np.int64)        # exact scaling, ties to even
            row[s0:s0 + NJ] += fixed
            bins = np.clip(np.floor((e * F(1000.0)).astype(F)).astype(np.int64), 0, BINS - 1)
            np.add.at(row, h0 + bins, 1)
    return table


def accumulate_case(B: int = 65, n_groups: int = 3, seed: int = 31):
    """(err_j, err_pa_j, group) with: group 1 empty, group -1 twice, a NaN pose, a pose with one value 2e3, and values of exactly
    0.05f, 0.15f and 0.1499999f"""
    rs = np.random.RandomState(seed)
    e0 = np.abs(rs.randn(B, NJ) * 0.06).astype(F)
    e1 = np.abs(rs.randn(B, NJ) * 0.03).astype(F)
    group = np.where(rs.rand(B) < 0.5, 0, 2).astype(np.int32)
    group[[5, 44]] = -1
    e0[7, 3] = np.nan
    e1[50, 16] = F(2e3)
    e0[1, 0], e0[1, 1], e0[1, 2] = F(0.05), F(0.15), F(0.1499999)
    e1[60, 4], e1[60, 5], e1[60, 6] = F(0.05), F(0.15), F(0.1499999)
    e0[2, 0] = np.inf
    e0[3, 1] = F(999.9)                           # absurd but below the cap: counted, bin 150
    return e0, e1, group


# ---- what tests/golden/g10_eval_joints.npz was computed on (tests/golden/make_golden_eval.py) --------------------------------
G10_POSES, G10_POSE_SEED = 65, 11
G10_MESHES, G10_MESH_SEED, G10_DENSE_SEED, G10_ZERO_ROW = 3, 21, 22, 5
