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
