"""Host restatement and cases of the bone length and direction errors (jrr_bone_error, jrr_bone_accumulate; bones_report).

Written from include/jrr.h: the parent table, the six left / right pairs, the 98 values per pose (every operation rounded once in the
order written -- numpy's arithmetic in one dtype does exactly that), the table layout JRR_BONE_ACC_* and what a pose adds to it.
Evaluable in float32 (the kernel's format; the rotation is eval_report_cases.kernel_rotation, the statements of csrc/procfit.h) and in
float64 (the yardstick; the rotation is V diag(1, 1, sign det(U V^T)) U^T from numpy's float64 SVD of the float64 moments).  There is no
reference implementation, so a comparison is held to accel_cases.bound = 3 x max|f32 - f64| + 1e-7 of the restatement's two evaluations
on the test's OWN inputs, never to anything the kernel returned; the two angle blocks get 4 x 2^-23 x pi rad more for the device's
atan2f (ANGLE_SLACK).
"""
import numpy as np

import accel_cases as ac
import eval_report_cases as erc

F, F64 = np.float32, np.float64
NJ, NB, NP = 17, 16, 6
PARENT = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)
PAIRS = ((4, 1), (5, 2), (6, 3), (11, 14), (12, 15), (13, 16))
PAIR_NAMES = ('pelvis-hip', 'thigh', 'shin', 'neck-shoulder', 'upper arm', 'forearm')
VALS, LEN_PRED, LEN_GT, ANG, ANG_PA, ERR_DIR, ERR_LEN = 98, 0, 16, 32, 48, 64, 81
BLOCKS = (('len_pred', LEN_PRED, NB), ('len_gt', LEN_GT, NB), ('ang', ANG, NB), ('ang_pa', ANG_PA, NB), ('e_dir', ERR_DIR, NJ),
          ('e_len', ERR_LEN, NJ))
ROW, TRAILER = 192, 2
(COUNT, BAD, SUM_LEN_PRED, SUM_LEN_GT, SUM_ABS_DLEN, SUM_ANG, SUM_ANG_PA, SUM_SQ_PRED, SUM_SQ_GT, SUM_Q_PRED, SUM_Q_GT, SUM_ERR_DIR, SUM_ERR_LEN,
 SUM_ASYM_PRED, SUM_ASYM_GT) = 0, 1, 2, 18, 34, 50, 66, 82, 98, 114, 130, 146, 163, 180, 186
ANGLE_SLACK = 4.0 * 2.0 ** -23 * np.pi             # the device's atan2f against numpy's
bound, dist = ac.bound, ac.dist


# ---- the restatement -------------------------------------------------------------------------------------------------------
def _len(w):
    return np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _angle(a, b):
    return np.arctan2(_len(_cross(a, b)), _dot(a, b))


def centred(pred, gt_mm, dtype):
    """(x, y) (B,17,3) in `dtype`: x = P - P[0], y = G / 1000 - (G / 1000)[0]"""
    P, G = np.asarray(pred, dtype=F).astype(dtype), np.asarray(gt_mm, dtype=F).astype(dtype)
    q = G / dtype(1000)
    return P - P[:, :1], q - q[:, :1]


def moments(x, y):
    """(K (B,3,3), var1 (B,), mu1, mu2 (B,3)) in the statement order of eval_report_cases.kernel_evaluate_joints"""
    dtype = x.dtype.type
    B = x.shape[0]
    mu1, mu2 = np.zeros((B, 3), dtype=dtype), np.zeros((B, 3), dtype=dtype)
    for i in range(NJ):
        mu1, mu2 = mu1 + x[:, i], mu2 + y[:, i]
    mu1, mu2 = mu1 / dtype(NJ), mu2 / dtype(NJ)
    K, var1 = np.zeros((B, 3, 3), dtype=dtype), np.zeros(B, dtype=dtype)
    for i in range(NJ):
        x1, x2 = x[:, i] - mu1, y[:, i] - mu2
        for c in range(3):
            var1 = var1 + x1[:, c] * x1[:, c]
        for r in range(3):
            for c in range(3):
                K[:, r, c] = K[:, r, c] + x1[:, r] * x2[:, c]
    return K, var1, mu1, mu2


def rotation(K):
    """R (B,3,3) in K's dtype.  float32: the statements of csrc/procfit.h.  float64: V diag(1, 1, sign det(U V^T)) U^T (eval_utils.py:38-44
    of the reference) from numpy's SVD; a K that is not finite gives NaN."""
    if K.dtype == F:
        return erc.kernel_rotation(K)
    R = np.full(K.shape, np.nan)
    ok = np.isfinite(K).all(axis=(1, 2))
    if ok.any():
        U, _, Vt = np.linalg.svd(K[ok])
        V = np.swapaxes(Vt, 1, 2)
        Z = np.broadcast_to(np.eye(3), U.shape).copy()
        Z[:, 2, 2] = np.sign(np.linalg.det(U @ Vt))
        R[ok] = V @ Z @ np.swapaxes(U, 1, 2)
    return R


def bones(pred, gt_mm, dtype=F64):
    """(B,98) in `dtype`: the definition of include/jrr.h, each operation once, in order"""
    x, y = centred(pred, gt_mm, dtype)
    B = x.shape[0]
    out = np.zeros((B, VALS), dtype=dtype)
    with np.errstate(all='ignore'):
        K, _, _, _ = moments(x, y)
        R = rotation(K)
        xd, xl = np.zeros_like(x), np.zeros_like(x)
        for b in range(1, NJ):
            p = PARENT[b]
            u, v = x[:, b] - x[:, p], y[:, b] - y[:, p]
            lp, lg = _len(u), _len(v)
            ru = np.stack([(R[:, r, 0] * u[:, 0] + R[:, r, 1] * u[:, 1]) + R[:, r, 2] * u[:, 2] for r in range(3)], 1)
            out[:, LEN_PRED + b - 1], out[:, LEN_GT + b - 1] = lp, lg
            out[:, ANG + b - 1], out[:, ANG_PA + b - 1] = _angle(u, v), _angle(ru, v)
            sd, sl = lg / lp, lp / lg
            xd[:, b] = xd[:, p] + u * sd[:, None]
            xl[:, b] = xl[:, p] + v * sl[:, None]
            out[:, ERR_DIR + b], out[:, ERR_LEN + b] = _len(xd[:, b] - y[:, b]), _len(xl[:, b] - y[:, b])
    assert out.dtype == dtype
    return out


def block(vals, name):
    _, at, n = next(b for b in BLOCKS if b[0] == name)
    return vals[:, at:at + n]


def block_bounds(r32, r64, rows=None, rows_pa=None):
    """name -> bound of the block on `rows` (None: all; `ang_pa` on rows_pa), the angle blocks with ANGLE_SLACK"""
    out = {}
    for name, _, _ in BLOCKS:
        sel = rows_pa if name == 'ang_pa' and rows_pa is not None else rows
        a, b = block(r32, name), block(r64, name)
        if sel is not None:
            a, b = a[sel], b[sel]
        out[name] = bound(a, b) + (ANGLE_SLACK if name.startswith('ang') else 0.0)
    return out


# ---- the table in Python integers ------------------------------------------------------------------------------------------
def _fixed(v, scale=16777216.0):
    """llrintf(v * scale): the product is exact (a power of two), the rounding to nearest, ties to even"""
    return int(np.rint(np.float64(np.float32(v) * F(scale))))


def accumulate(vals, group, n_groups, table=None):
    """ADD to `table` (a list of Python integers, n_groups * 192 + 2; None = zeros) what jrr_bone_accumulate adds for the float32 rows
    `vals` (B,98); returns the list"""
    vals = np.asarray(vals)
    assert vals.dtype == F and vals.shape[1] == VALS
    table = [0] * (n_groups * ROW + TRAILER) if table is None else [int(w) for w in table]
    group = np.zeros(vals.shape[0], dtype=np.int64) if group is None else np.asarray(group).astype(np.int64)
    for b in range(vals.shape[0]):
        g, v = int(group[b]), vals[b]
        if g < 0:
            table[n_groups * ROW] += 1
            continue
        if g >= n_groups:
            table[n_groups * ROW + 1] += 1
            continue
        r0 = g * ROW
        with np.errstate(invalid='ignore'):
            good = bool((v < F(1.0e3)).all())
        if not good:
            table[r0 + BAD] += 1
            continue
        table[r0 + COUNT] += 1
        for i in range(NB):
            lp, lg = v[LEN_PRED + i], v[LEN_GT + i]
            table[r0 + SUM_LEN_PRED + i] += _fixed(lp)
            table[r0 + SUM_LEN_GT + i] += _fixed(lg)
            table[r0 + SUM_ABS_DLEN + i] += _fixed(np.abs(lp - lg))
            table[r0 + SUM_ANG + i] += _fixed(v[ANG + i])
            table[r0 + SUM_ANG_PA + i] += _fixed(v[ANG_PA + i])
            table[r0 + SUM_SQ_PRED + i] += _fixed(lp, 65536.0) ** 2
            table[r0 + SUM_SQ_GT + i] += _fixed(lg, 65536.0) ** 2
            table[r0 + SUM_Q_PRED + i] += _fixed(lp, 65536.0)
            table[r0 + SUM_Q_GT + i] += _fixed(lg, 65536.0)
        for j in range(NJ):
            table[r0 + SUM_ERR_DIR + j] += _fixed(v[ERR_DIR + j])
            table[r0 + SUM_ERR_LEN + j] += _fixed(v[ERR_LEN + j])
        for k, (left, right) in enumerate(PAIRS):
            table[r0 + SUM_ASYM_PRED + k] += _fixed(np.abs(v[LEN_PRED + left - 1] - v[LEN_PRED + right - 1]))
            table[r0 + SUM_ASYM_GT + k] += _fixed(np.abs(v[LEN_GT + left - 1] - v[LEN_GT + right - 1]))
    return table


def as_int64(table):
    assert all(-(1 << 63) <= w < (1 << 63) for w in table)
    return np.array(table, dtype=np.int64)


def host_bone_error(pred, gt_mm, out=None):
    """engine.bone_error on CPU tensors by the float32 restatement (the GPU tests hold the kernel to it)"""
    import torch
    vals = torch.from_numpy(bones(pred.numpy(), gt_mm.numpy(), F))
    if out is None:
        return vals
    out.copy_(vals)
    return out


def host_bone_accumulate(vals, group, n_groups, acc):
    """engine.bone_accumulate on CPU tensors"""
    import torch
    acc.copy_(torch.from_numpy(as_int64(accumulate(vals.numpy(), None if group is None else group.numpy(), int(n_groups), acc.numpy().tolist()))))


# ---- cases -----------------------------------------------------------------------------------------------------------------
def dyadic_poses(n=12, seed=1, multiple=1):
    """gt_mm (n,17,3) float32 and its metres (n,17,3) float64: every coordinate is multiple * k / 1024 m with |k| <= 128 and the ground
    truth is 1000 x that, so that G / 1000, every difference, every product of two differences and the sums of three of them are exact in
    float32 (pattern: accel_cases.dyadic_track).  The pelvis is not at the origin."""
    rng = np.random.RandomState(seed)
    m = multiple * rng.randint(-128, 129, size=(n, NJ, 3)) / 1024.0
    for b in range(1, NJ):                          # no bone of length 0
        same = (m[:, b] == m[:, PARENT[b]]).all(1)
        m[same, b, 0] += multiple * 8 / 1024.0
    gt = (m * 1000.0).astype(F)
    assert np.array_equal(gt.astype(F64), m * 1000.0) and np.array_equal((gt / F(1000)).astype(F64), m)
    return gt, m


GPU_FAMILIES = ('flat_target', 'flat_pred', 'flat_both_mirrored', 'collinear_pred', 'collinear_target')
COLLINEAR = ('collinear_pred', 'collinear_target')
GPU_POOL = 257
GPU_BATCHES = (1, 63, 64, 65, 257)


def gpu_pool(n=GPU_POOL):
    """(pred (n,17,3), gt_mm (n,17,3), collinear (n,) bool): pose i is pose i // 6 of source i mod 6 -- eval_report_cases.pose_cases, then
    its flat and collinear families -- so that every wave holds every shape.  collinear: the poses on which ang_pa is not defined."""
    per = (n + 5) // 6
    src = [erc.pose_cases(per, 41)] + [erc.family_cases(k, per) for k in GPU_FAMILIES]
    which, row = np.arange(n) % 6, np.arange(n) // 6
    pred = np.stack([src[w][0][r] for w, r in zip(which, row)])
    gt = np.stack([src[w][1][r] for w, r in zip(which, row)])
    collinear = np.isin(which, [1 + GPU_FAMILIES.index(k) for k in COLLINEAR])
    return pred, gt, collinear


def table_case(n=65, n_groups=3, seed=5):
    """(pred, gt_mm, group, special) for the table checks: body-shaped poses in groups 0 and 2 (group 1 stays empty), two poses with
    group -1, one with group n_groups, and -- each in a group of its own right -- a NaN pose, a pose whose predicted joint 5 coincides
    with its parent, and a constant pred.  special: name -> pose index."""
    pred, gt = erc.family_cases('body', n, seed)
    rng = np.random.RandomState(seed)
    group = np.where(rng.rand(n) < 0.5, 0, 2).astype(np.int32)
    special = {'ignored_a': 5, 'ignored_b': 44, 'bad_group': 20, 'nan': 7, 'zero_bone': 33, 'constant_pred': 50}
    group[[5, 44]] = -1
    group[20] = n_groups
    pred, gt = pred.copy(), gt.copy()
    gt[7, 3, 1] = np.nan
    pred[33, 5] = pred[33, PARENT[5]]
    pred[50] = pred[50, 3]
    return pred, gt, group, special


def frame_path(subject, action, camera, frame):
    return f'/data/h36m/{subject}/{action}/imageSequence/{camera}/img_{frame:06d}.jpg'


def rigid_dataset(n=40, seed=3):
    """(gt_mm (n,17,3) float32, paths): two subjects (S9: samples 0 .. n/2 - 1, S11: the rest), each ONE rigid skeleton translated by
    dyadic offsets (no rotation: every bone vector keeps its bits, so the ground truth's rigidity is exactly 0), two actions"""
    rng = np.random.RandomState(seed)
    gt = np.zeros((n, NJ, 3), dtype=F)
    paths = []
    for s, (name, lo, hi) in enumerate((('S9', 0, n // 2), ('S11', n // 2, n))):
        skel, _ = dyadic_poses(1, seed + s)
        for i in range(lo, hi):
            off = rng.randint(-64, 65, size=(1, 3)) / 1024.0 * 1000.0
            gt[i] = (skel[0].astype(F64) + off).astype(F)
            paths.append(frame_path(name, 'Walking 1' if i % 2 else 'Eating', 1, 5 * (i + 1)))
    return gt, paths


def report_case(n=40):
    """(before, after (n,17,3) m, gt_mm, paths): rigid_dataset, and two predictions around it -- 1.1 x the truth with 20 mm of noise,
    the truth with 5 mm"""
    gt, paths = rigid_dataset(n)
    rng = np.random.RandomState(4)
    m = gt.astype(F64) / 1000.0
    before = (m * 1.1 + rng.normal(0, 0.02, size=m.shape)).astype(F)
    after = (m + rng.normal(0, 0.005, size=m.shape)).astype(F)
    return before, after, gt, paths


def fill(report, before, after, gt, gids, sids, lo, hi, batch=16):
    """add poses [lo, hi) to a bones_report.BoneReport on the CPU, in batches"""
    import torch
    for a in range(lo, hi, batch):
        b = min(a + batch, hi)
        g, s = torch.from_numpy(gids[a:b].copy()), (None if sids is None else torch.from_numpy(sids[a:b].copy()))
        report.add('before', torch.from_numpy(before[a:b]), torch.from_numpy(gt[a:b]), g, s)
        report.add('after', torch.from_numpy(after[a:b]), torch.from_numpy(gt[a:b]), g, s)
