"""Host restatement of the evaluation protocols (tests/test_eval_protocol.py, tests/test_gpu_eval_protocol.py,
tests/golden/make_golden_protocol.py): jrr_evaluate_protocol of include/jrr.h in torch, in a dtype of the caller's choice, and its
masked accumulate in exact integers.

The protocol: centre both skeletons on the root (joint 0, or the midpoint of joints 1 and 4), select the joints of the mask, apply
eval_report_cases.procrustes -- the reference's N-agnostic batch_compute_similarity_transform_torch (scripts/eval_utils.py:7-58) -- to
the selection.  Excluded columns hold 0.

Bounds: eval_report_cases.bound(d) = 3 d + 1e-7 with d the distance of the float32 restatement from the float64 one on the test's own
inputs; no value is excluded from a comparison."""
import numpy as np
import torch

import eval_report_cases as ec

F = np.float32
NJ = ec.NJ
ROOT_JOINT0, ROOT_HIPS = 0, 1
TARGET_MM, TARGET_M = 0, 1
ROOTS = {'joint0': ROOT_JOINT0, 'hips': ROOT_HIPS}


def mask_of(joints) -> int:
    return sum(1 << int(j) for j in joints)


def joints_of(mask: int):
    return [i for i in range(NJ) if mask >> i & 1]


MASKS = {
    'all17': mask_of(range(17)),
    'lsp14': mask_of([1, 2, 3, 4, 5, 6, 8, 10, 11, 12, 13, 14, 15, 16]),
    'limbs12': mask_of([1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 15, 16]),
    'tri3': mask_of([1, 4, 8]),          # three points: K has rank 2
    'pair2': mask_of([3, 10]),           # two points: rank 1
    'one1': mask_of([10]),               # one point: var1 = 0, the reference's aligned distance is 0/0 = NaN, the plain one finite
}
G13_MASKS = ('lsp14', 'tri3', 'pair2')   # in tests/golden/g13_eval_protocol.npz, each with both roots, on g11's 48 poses


def g13_key(mask_name: str, root_name: str, what: str) -> str:
    return f'{what}_{mask_name}_{root_name}'


def evaluate_protocol(pred, target, mask: int, root: int, unit: int = TARGET_MM, dtype=torch.float32, procrustes=ec.procrustes):
    """(err_j (B,17), err_pa_j (B,17)) in metres, numpy in `dtype`, 0 in the columns outside the mask.  pred (B,17,3) m, target
    (B,17,3) in `unit`; `procrustes`: the similarity fit of (B,n,3) onto (B,n,3) (the golden generator passes the reference's own)"""
    p = torch.as_tensor(np.asarray(pred)).to(dtype)
    t = torch.as_tensor(np.asarray(target)).to(dtype)
    if unit == TARGET_MM:
        t = t / 1000
    if root == ROOT_JOINT0:
        p = p - p[:, [0], :]
        t = t - t[:, [0], :]
    else:
        p = p - (p[:, [1], :] + p[:, [4], :]) * 0.5
        t = t - (t[:, [1], :] + t[:, [4], :]) * 0.5
    sel = joints_of(mask)
    p, t = p[:, sel, :].contiguous(), t[:, sel, :].contiguous()
    e = torch.sqrt(((p - t) ** 2).sum(dim=-1))
    e_pa = torch.sqrt(((procrustes(p, t) - t) ** 2).sum(dim=-1))
    err_j, err_pa_j = torch.zeros(p.shape[0], NJ, dtype=dtype), torch.zeros(p.shape[0], NJ, dtype=dtype)
    err_j[:, sel], err_pa_j[:, sel] = e, e_pa
    return err_j.numpy(), err_pa_j.numpy()


def distance(a32, a64) -> float:
    """the largest |a32 - a64| over the entries that are finite in both; the NaN patterns must agree (asserted)"""
    a32, a64 = np.asarray(a32, dtype=np.float64), np.asarray(a64, dtype=np.float64)
    assert np.array_equal(np.isnan(a32), np.isnan(a64)), 'NaN patterns of float32 and float64 differ'
    both = ~np.isnan(a64)
    return float(np.abs(a32[both] - a64[both]).max()) if both.any() else 0.0


def accumulate(err_j, err_pa_j, group, n_groups: int, mask: int, table=None) -> np.ndarray:
    """ADD to `table` (int64, n_groups * 338 + 2; None = zeros) what jrr_evaluate_protocol adds for the joints of `mask`, in exact
    integers: eval_report_cases.accumulate with every loop over the 17 joints run over the mask alone"""
    ROW, TRAILER, BINS = ec.ROW, ec.TRAILER, ec.BINS
    table = np.zeros(n_groups * ROW + TRAILER, dtype=np.int64) if table is None else table.copy()
    e0, e1 = np.asarray(err_j, dtype=F), np.asarray(err_pa_j, dtype=F)
    sel = np.array(joints_of(mask))
    group = np.zeros(e0.shape[0], dtype=np.int32) if group is None else np.asarray(group)
    for b, g in enumerate(group.tolist()):
        if g < 0:
            table[n_groups * ROW + 0] += 1
            continue
        if g >= n_groups:
            table[n_groups * ROW + 1] += 1
            continue
        row = table[g * ROW:(g + 1) * ROW]
        with np.errstate(invalid='ignore'):
            good = bool(np.all(e0[b, sel] < F(1.0e3)) and np.all(e1[b, sel] < F(1.0e3)))
        if not good:
            row[ec.BAD] += 1
            continue
        row[ec.COUNT] += 1
        for e, s0, h0 in ((e0[b, sel], ec.SUM, ec.HIST), (e1[b, sel], ec.SUM_PA, ec.HIST_PA)):
            fixed = np.rint((e * F(16777216.0)).astype(F).astype(np.float64)).astype(np.int64)        # exact scaling, ties to even
            np.add.at(row, s0 + sel, fixed)
            bins = np.clip(np.floor((e * F(1000.0)).astype(F)).astype(np.int64), 0, BINS - 1)
            np.add.at(row, h0 + bins, 1)
    return table


def means_mm(table: np.ndarray, n_groups: int, mask: int):
    """(n (G,), MPJPE (G,), PA-MPJPE (G,)) in mm, float64, from a table: sum / 2^24 / (n_joints count) * 1000"""
    rows = np.asarray(table)[:n_groups * ec.ROW].reshape(n_groups, ec.ROW)
    n = rows[:, ec.COUNT].astype(np.float64)
    nj = len(joints_of(mask))
    with np.errstate(all='ignore'):
        return (rows[:, ec.COUNT], rows[:, ec.SUM:ec.SUM + NJ].sum(1) / float(1 << 24) / (nj * n) * 1000.0,
                rows[:, ec.SUM_PA:ec.SUM_PA + NJ].sum(1) / float(1 << 24) / (nj * n) * 1000.0)
