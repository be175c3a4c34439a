"""Host restatement and seeded inputs of the per-vertex error (tests/test_vertex_error.py, tests/test_gpu_vertex_error.py,
tests/golden/make_golden_pve.py).

Written from include/jrr.h (jrr_vertex_error, JRR_PVE_ACC_*), which is the specification, and from the reference's
batch_compute_similarity_transform_torch (scripts/eval_utils.py:7-58) for the float64 yardstick.  Meshes are regenerated from
numpy.random.RandomState seeds here, never stored.

Bounds: `bound(d) = max(FLOOR, 1.5 d)`, d the distance of the float32 restatement below from the float64
evaluation ON THE TEST'S OWN INPUTS, the floor the reference's own float32 distance from float64 on the families of the fixture as
tests/golden/make_golden_pve.py printed it, rounded up to one digit.  Measured against float64, never against the kernel."""
import numpy as np
import torch

import eval_report_cases as ec

F, F64 = np.float32, np.float64
ROW, TRAILER, MAX_PARTS = 370, 2, 32
COUNT, BAD, SUM, SUM_PA, HIST, HIST_PA, PART, PART_PA, BINS = 0, 1, 2, 3, 4, 155, 306, 338, 151
FIXED = 16777216.0
BODY = (0.15, 0.5, 0.05)                               # extents of a standing body in metres
FAMILIES = {'body': 41, 'similarity_copy': 42, 'flat_target': 43, 'mirrored_pred': 44, 'constant_target': 45}      # name -> seed
G12_VERTS = (3, 65, 431, 6890)
G12_POSES = 4
SUBSET = 512                                           # vertices of a 6890-vertex mesh whose values the fixture keeps
# what tests/golden/make_golden_pve.py printed for the reference's float32 evaluation against float64 over all of the fixture's
# cases (the maximum over families and vertex counts), rounded up to one digit: per-vertex values, per-pose means
FLOOR_VERTEX, FLOOR_POSE = 2e-6, 4e-7


def bound(d: float, floor: float) -> float:
    return max(float(floor), 1.5 * float(d))


def dist(a, b) -> float:
    """max |a - b| over the entries where b is finite; NaN patterns are compared separately"""
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    m = np.isfinite(b)
    return float(np.abs(a[m] - b[m]).max()) if m.any() else 0.0


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------
def family_case(name: str, n_verts: int, B: int = G12_POSES, seed=None):
    """(pred, gt (B,n_verts,3), root_pred, root_gt (B,3)) float32 metres.  gt is a body-shaped cloud (sigma 0.15 / 0.5 / 0.05 m) in a
    random rigid frame, away from the origin; pred is a similarity transform of it (scale 0.8 .. 1.2, a large rotation, a shift)
    plus 2 cm noise -- `similarity_copy`: no noise; `flat_target`: the target's thin axis exactly zero before its rotation;
    `mirrored_pred`: the pred mirrored in x before its rotation; `constant_target`: every target vertex the first one.  The roots
    are points near the meshes (what a pelvis joint would be), not vertices."""
    seed = FAMILIES[name] * 100003 + n_verts if seed is None else seed
    rs = np.random.RandomState(seed)
    base = rs.randn(B, n_verts, 3) * np.asarray(BODY)
    if name == 'flat_target':
        base[:, :, 2] = 0
    R0, R1 = ec._rodrigues(rs.randn(B, 3) * 2.0), ec._rodrigues(rs.randn(B, 3) * 2.0)
    gt = np.einsum('brc,bic->bir', R0, base) + rs.randn(B, 1, 3) * 0.5
    src = base.copy()
    if name == 'mirrored_pred':
        src[:, :, 0] *= -1
    scale = 0.8 + 0.4 * rs.rand(B, 1, 1)
    noise = 0.0 if name == 'similarity_copy' else 0.02
    pred = scale * np.einsum('brc,bic->bir', R1 @ R0, src) + rs.randn(B, 1, 3) * 0.5 + rs.randn(B, n_verts, 3) * noise
    if name == 'constant_target':
        gt[:] = gt[:, [0], :]
    root_pred = pred.mean(1) + rs.randn(B, 3) * 0.05
    root_gt = gt.mean(1) + rs.randn(B, 3) * 0.05
    return pred.astype(F), gt.astype(F), root_pred.astype(F), root_gt.astype(F)


def mixed_case(n_verts: int, B: int, seed: int = 7):
    """B poses that cycle through the families, in one batch"""
    names = list(FAMILIES)
    per = {k: family_case(k, n_verts, (B + len(names) - 1) // len(names), seed=seed * 1009 + FAMILIES[k] * 31 + n_verts) for k in names}
    fam, row = np.arange(B) % len(names), np.arange(B) // len(names)
    return tuple(np.stack([per[names[f]][k][r] for f, r in zip(fam, row)]) for k in range(4)) + (fam,)


def subset(n_verts: int) -> np.ndarray:
    """the vertices whose per-vertex values tests/golden/g12_vertex_error.npz keeps: all of a small mesh, 512 seeded ones of a large one"""
    if n_verts <= SUBSET:
        return np.arange(n_verts)
    return np.sort(np.random.RandomState(12).choice(n_verts, SUBSET, replace=False))


# ---- the float64 yardstick ---------------------------------------------------------------------------------------------------
def evaluate64(pred, gt, root_pred=None, root_gt=None):
    """(d (B,n), e (B,n), pve (B,), pa_pve (B,)) float64 metres: the definition in float64 from the float32 inputs, the alignment by
    the reference's lines (torch.svd and the det-sign fix)"""
    x = np.asarray(pred, dtype=F64) - (0 if root_pred is None else np.asarray(root_pred, dtype=F64)[:, None, :])
    y = np.asarray(gt, dtype=F64) - (0 if root_gt is None else np.asarray(root_gt, dtype=F64)[:, None, :])
    d = np.sqrt(((x - y) ** 2).sum(-1))
    with np.errstate(all='ignore'):
        hat = ec.procrustes(torch.from_numpy(x), torch.from_numpy(y)).numpy()
    e = np.sqrt(((hat - y) ** 2).sum(-1))
    return d, e, d.mean(1), e.mean(1)


# ---- the float32 restatement of include/jrr.h ----------------------------------------------------------------------------------
def fixed(v) -> np.ndarray:
    """llrintf(v * 2^24) of float32 values (ties to even), int64; 0 where v fails v < 1.0e3f"""
    v = np.asarray(v, dtype=F)
    with np.errstate(invalid='ignore'):
        ok = v < F(1.0e3)
    return np.where(ok, np.rint((np.where(ok, v, F(0)) * F(FIXED)).astype(F).astype(F64)), 0).astype(np.int64)


def pose_mean(v) -> np.ndarray:
    """(B,) float32: (float)((double)S / ((double)n * 2^24)), NaN where a value fails v < 1.0e3f"""
    v = np.asarray(v, dtype=F)
    with np.errstate(invalid='ignore'):
        ok = (v < F(1.0e3)).all(1)
    S = fixed(v).sum(1)
    return np.where(ok, (S.astype(F64) / (F64(v.shape[1]) * FIXED)).astype(F), F(np.nan)).astype(F)


def restate(pred, gt, root_pred=None, root_gt=None):
    """(d, e (B,n) float32, pve, pa_pve (B,) float32) as include/jrr.h states them: every float32 operation rounded once in the order
    written; the moments in float64 (numpy's summation order, not the kernel's: they agree to a few 1e-16 relative before the
    rounding to float32) about the float64 means; the rotation by eval_report_cases.kernel_rotation, the float32 restatement of
    csrc/evalk.h"""
    P, Q = np.asarray(pred, dtype=F), np.asarray(gt, dtype=F)
    B, n = P.shape[:2]
    x = P - (np.zeros((B, 3), F) if root_pred is None else np.asarray(root_pred, dtype=F))[:, None, :]
    y = Q - (np.zeros((B, 3), F) if root_gt is None else np.asarray(root_gt, dtype=F))[:, None, :]
    assert x.dtype == F and y.dtype == F
    with np.errstate(all='ignore'):
        df = x - y
        d = np.sqrt((df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2])
        x64, y64 = x.astype(F64), y.astype(F64)
        m1, m2 = x64.sum(1) / n, y64.sum(1) / n
        a, c = x64 - m1[:, None, :], y64 - m2[:, None, :]
        K = np.einsum('bir,bic->brc', a, c).astype(F)
        var1 = ((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]).sum(1).astype(F)
        mu1, mu2 = m1.astype(F), m2.astype(F)
        R = ec.kernel_rotation(K)
        tr = np.zeros(B, dtype=F)
        for r in range(3):
            tr = tr + (R[:, r, 0] * K[:, 0, r] + R[:, r, 1] * K[:, 1, r] + R[:, r, 2] * K[:, 2, r])
        scale = tr / var1
        t = np.stack([mu2[:, r] - scale * (R[:, r, 0] * mu1[:, 0] + R[:, r, 1] * mu1[:, 1] + R[:, r, 2] * mu1[:, 2]) for r in range(3)], 1)
        d2 = np.zeros((B, n), dtype=F)
        for r in range(3):
            h = scale[:, None] * (R[:, None, r, 0] * x[..., 0] + R[:, None, r, 1] * x[..., 1] + R[:, None, r, 2] * x[..., 2]) + t[:, None, r]
            dd = h - y[..., r]
            d2 = d2 + dd * dd
        e = np.sqrt(d2)
    assert d.dtype == F and e.dtype == F and scale.dtype == F and t.dtype == F
    return d, e, pose_mean(d), pose_mean(e)


# ---- restatement: the tables ----------------------------------------------------------------------------------------------------
def accumulate(err_v, err_pa_v, pve, pa_pve, group, n_groups: int, part=None, n_parts: int = 0, table=None, table_v=None):
    """ADD to (`table` int64 n_groups * 370 + 2, `table_v` int64 (2,n); None = zeros) what jrr_vertex_error adds for poses with these
    float32 outputs, in exact integers"""
    d, e = np.asarray(err_v, dtype=F), np.asarray(err_pa_v, dtype=F)
    B, n = d.shape
    table = np.zeros(n_groups * ROW + TRAILER, dtype=np.int64) if table is None else table.copy()
    table_v = np.zeros((2, n), dtype=np.int64) if table_v is None else table_v.copy()
    group = np.zeros(B, dtype=np.int64) if group is None else np.asarray(group)
    for b in range(B):
        g = int(group[b])
        if g < 0:
            table[n_groups * ROW + 0] += 1
            continue
        if g >= n_groups:
            table[n_groups * ROW + 1] += 1
            continue
        row = table[g * ROW:(g + 1) * ROW]
        if np.isnan(pve[b]) or np.isnan(pa_pve[b]):
            row[BAD] += 1
            continue
        row[COUNT] += 1
        for v, m, s0, h0, p0, k in ((d[b], pve[b], SUM, HIST, PART, 0), (e[b], pa_pve[b], SUM_PA, HIST_PA, PART_PA, 1)):
            q = fixed(v)
            row[s0] += int(fixed(np.array([m]))[0])
            row[h0 + min(int(np.floor(F(m) * F(1000.0))), BINS - 1)] += 1
            table_v[k] += q
            if part is not None:
                for p in range(n_parts):
                    sel = np.asarray(part) == p
                    if sel.any():
                        mp = F(F64(int(q[sel].sum())) / (F64(int(sel.sum())) * FIXED))
                        row[p0 + p] += int(fixed(np.array([mp]))[0])
    return table, table_v
