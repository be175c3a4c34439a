"""Host restatement and cases of the time-axis filter over the refined-pose table (jrr_pose_smooth, jrr_pose_jitter; refined.smooth).

Written from the definitions include/jrr.h states for the two entry points and from the reference's rot6d_to_rotmat
(scripts/utils.py:198-204), in numpy for a chosen dtype.  There is no reference implementation: the yardstick is float64.  The
distance of the float32 evaluation of these functions from their float64 evaluation, on a test's own inputs, is what the GPU is held
to: `bound(d) = 3 d + 1e-7` (tests/refined_cases.py).  Rotations are compared as matrices, angles in radians; a
NaN must sit where the float64 evaluation has one, and the maximum runs over every other entry.
"""
import numpy as np

N_ROWS, ROW = 96, 240
RUN_LENGTHS = (1, 2, 3, 33, 31)          # 70 positions: the last two runs and their windows straddle the 32-position tiles
M = sum(RUN_LENGTHS)
RADII = (0, 1, 6, 16)


def bound(d):
    return 3.0 * float(d) + 1e-7


def weights(sigma, radius):
    k = np.arange(radius + 1, dtype=np.float64)
    return np.exp(-(k * k) / (2.0 * float(sigma) ** 2)).astype(np.float32)


# ---- the restatement ------------------------------------------------------------------------------------------------------
def rot6d(x, dtype=np.float64):
    """(..., 6) -> (..., 3, 3): x.view(3, 2), a1 = x[:, 0], a2 = x[:, 1], b1 = normalize(a1), b2 = normalize(a2 - (b1 . a2) b1),
    b3 = b1 x b2, stacked as columns (F.normalize: v / max(|v|, 1e-12))"""
    x = np.asarray(x).astype(dtype)
    a1, a2 = x[..., 0::2], x[..., 1::2]
    eps = dtype(1e-12)
    with np.errstate(all='ignore'):
        b1 = a1 / np.maximum(np.sqrt((a1 * a1).sum(-1)), eps)[..., None]
        u = a2 - (b1 * a2).sum(-1)[..., None] * b1
        b2 = u / np.maximum(np.sqrt((u * u).sum(-1)), eps)[..., None]
    b3 = np.cross(b1, b2)
    return np.stack([b1, b2, b3], -1)


def unit_quat(R, dtype=np.float64):
    """(..., 3, 3) -> (..., 4) as (w, x, y, z): Shepperd's unnormalised quaternion -- of tr, R00, R11, R22 the largest, ties in that
    order -- divided by its norm"""
    R = np.asarray(R).astype(dtype)
    one = dtype(1)
    r = lambda i, j: R[..., i, j]
    r00, r11, r22 = r(0, 0), r(1, 1), r(2, 2)
    with np.errstate(all='ignore'):
        tr = r00 + r11 + r22
        c0 = (tr >= r00) & (tr >= r11) & (tr >= r22)
        c1 = ~c0 & (r00 >= r11) & (r00 >= r22)
        c2 = ~c0 & ~c1 & (r11 >= r22)
        quats = [(one + tr, r(2, 1) - r(1, 2), r(0, 2) - r(2, 0), r(1, 0) - r(0, 1)),
                 (r(2, 1) - r(1, 2), one + r00 - r11 - r22, r(0, 1) + r(1, 0), r(0, 2) + r(2, 0)),
                 (r(0, 2) - r(2, 0), r(0, 1) + r(1, 0), one + r11 - r00 - r22, r(1, 2) + r(2, 1)),
                 (r(1, 0) - r(0, 1), r(0, 2) + r(2, 0), r(1, 2) + r(2, 1), one + r22 - r00 - r11)]
        q = np.stack([np.where(c0, quats[0][k], np.where(c1, quats[1][k], np.where(c2, quats[2][k], quats[3][k]))) for k in range(4)], -1)
        q = q / np.sqrt((q * q).sum(-1))[..., None]
    assert q.dtype == dtype
    return q


def conj_mul(a, b):
    """conj(a) (x) b = (a . b,  a_w b_v - b_w a_v - a_v x b_v)"""
    aw, av, bw, bv = a[..., :1], a[..., 1:], b[..., :1], b[..., 1:]
    return np.concatenate([(a * b).sum(-1, keepdims=True), aw * bv - bw * av - np.cross(av, bv)], -1)


def angle_deg(e):
    dtype = e.dtype.type
    with np.errstate(all='ignore'):
        return dtype(2) * np.arctan2(np.sqrt((e[..., 1:] ** 2).sum(-1)), np.abs(e[..., 0])) * dtype(180.0 / np.pi)


def quat_to_6d(q):
    """the first two columns of R(q) in the 6-D layout: x[0], x[2], x[4] column 0, x[1], x[3], x[5] column 1"""
    dtype = q.dtype.type
    one, two = dtype(1), dtype(2)
    w, x, y, z = (q[..., k] for k in range(4))
    c0 = [one - two * (y * y + z * z), two * (x * y + w * z), two * (x * z - w * y)]
    c1 = [two * (x * y - w * z), one - two * (x * x + z * z), two * (y * z + w * x)]
    return np.stack([c0[0], c1[0], c0[1], c1[1], c0[2], c1[2]], -1)


def _mean_over_joints(a):
    """summed in joint order, then divided by the number of joints"""
    s = a[..., 0]
    for j in range(1, a.shape[-1]):
        s = s + a[..., j]
    return s / a.dtype.type(a.shape[-1])


def smooth(x6d, betas, cam, run, w, dtype=np.float64, valid=None):
    """the filter over positions: x6d (M,J,6), betas (M,10), cam (M,3), run (M,), w (radius+1,) float32, valid (M,) bool (a position
    that is not valid is nobody's neighbour and its outputs are NaN) -> (x6d_out, betas_out, cam_out, delta_deg) in `dtype`"""
    Mn, J = x6d.shape[0], x6d.shape[1]
    radius = len(w) - 1
    w = np.asarray(w, dtype=np.float32).astype(dtype)
    valid = np.ones(Mn, bool) if valid is None else np.asarray(valid, bool)
    q = unit_quat(rot6d(x6d, dtype), dtype)
    bc = np.concatenate([betas, cam], 1).astype(dtype)
    x_out, bc_out = np.full((Mn, J, 6), np.nan, dtype), np.full((Mn, bc.shape[1]), np.nan, dtype)
    delta = np.full(Mn, np.nan, dtype)
    with np.errstate(all='ignore'):
        for p in range(Mn):
            if not valid[p]:
                continue
            s, acc, wsum = np.zeros((J, 4), dtype), None, None
            for k in range(-radius, radius + 1):
                n = p + k
                if not (0 <= n < Mn) or run[n] != run[p] or not valid[n]:
                    continue
                qk = q[n]
                neg = (qk * q[p]).sum(-1) < 0
                s = s + w[abs(k)] * np.where(neg[:, None], -qk, qk)
                acc = w[abs(k)] * bc[n] if acc is None else acc + w[abs(k)] * bc[n]
                wsum = w[abs(k)] if wsum is None else wsum + w[abs(k)]
            s = s / np.sqrt((s * s).sum(-1))[:, None]
            x_out[p] = quat_to_6d(s)
            bc_out[p] = acc / wsum
            delta[p] = _mean_over_joints(angle_deg(conj_mul(q[p], s)))
    for a in (x_out, bc_out, delta):
        assert a.dtype == dtype
    return x_out, bc_out[:, :betas.shape[1]], bc_out[:, betas.shape[1]:], delta


def jitter(x6d, run, dtype=np.float64, valid=None):
    """(M,) in `dtype`: per position with both neighbours in its run the mean over the joints of the angle of
    e = conj(d1) (x) d2, d1 = conj(q[p-1]) (x) q[p], d2 = conj(q[p]) (x) q[p+1]; NaN elsewhere"""
    Mn = x6d.shape[0]
    valid = np.ones(Mn, bool) if valid is None else np.asarray(valid, bool)
    q = unit_quat(rot6d(x6d, dtype), dtype)
    out = np.full(Mn, np.nan, dtype)
    for p in range(1, Mn - 1):
        if run[p - 1] == run[p] == run[p + 1] and valid[p - 1] and valid[p] and valid[p + 1]:
            e = conj_mul(conj_mul(q[p - 1], q[p]), conj_mul(q[p], q[p + 1]))
            out[p] = _mean_over_joints(angle_deg(e))
    assert out.dtype == dtype
    return out


# ---- distances ------------------------------------------------------------------------------------------------------------
def dist(a, b):
    """max-abs distance over ALL entries; a NaN on one side only is an infinite distance, on both sides none"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    if (na != nb).any():
        return float('inf')
    return float(np.abs(np.where(na, 0.0, a) - np.where(nb, 0.0, b)).max()) if a.size else 0.0


def dist_rot(x6d_a, x6d_b):
    """smoothed rotations are compared as matrices (near pi two axis-angle vectors denote one rotation)"""
    return dist(rot6d(x6d_a, np.float64), rot6d(x6d_b, np.float64))


def dist_deg(a, b):
    """angles are compared in radians"""
    return dist(np.deg2rad(np.asarray(a, dtype=np.float64)), np.deg2rad(np.asarray(b, dtype=np.float64)))


# ---- cases ----------------------------------------------------------------------------------------------------------------
def expmap(aa):
    """float64 exact exponential map (n,3) -> (n,3,3)"""
    aa = np.asarray(aa, dtype=np.float64).reshape(-1, 3)
    th = np.linalg.norm(aa, axis=1)
    r = aa / np.where(th > 0, th, 1.0)[:, None]
    K = np.zeros((aa.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -r[:, 2], r[:, 1], r[:, 2], -r[:, 0], -r[:, 1], r[:, 0]
    sh = np.sin(0.5 * th)
    return np.eye(3)[None] + np.sin(th)[:, None, None] * K + (2 * sh * sh)[:, None, None] * (K @ K)


def to_6d(R):
    """(...,3,3) -> (...,6): the first two columns, x[2 i + k] = R[i, k]"""
    return np.asarray(R)[..., :, :2].reshape(*np.asarray(R).shape[:-2], 6)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def constant_velocity(T, axis, theta0, omega):
    """(T,6) float64: rotations by theta0 + omega t about one axis"""
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    return to_6d(expmap(axis[None] * (theta0 + omega * np.arange(T))[:, None]))


def sign_crossing(T, axis=(1.0, 2.0, -0.5), step=0.13):
    """(T,6) float64: a constant angular velocity about a fixed axis whose angle passes pi in mid-sequence, so the quaternion's w crosses
    0; from 25 frames on the ends lie below 1.6 rad, where Shepperd's choice falls on the trace: the branch differs along the sequence"""
    return constant_velocity(T, axis, np.pi - step * (T - 1) / 2, step)


def run_of_positions():
    return np.repeat(np.arange(len(RUN_LENGTHS)), RUN_LENGTHS).astype(np.int32)


def trajectories(seed, lengths=RUN_LENGTHS, J=24):
    """(sum lengths, J, 6) float32 in position order: per run and joint a trajectory with frame-to-frame noise; joint j % 4 selects
    0: any angle (a random base rotation times a constant velocity), 1: angles within 1e-3 of pi about a slowly moving axis,
    2: the exact identity, 3: the sign-crossing sequence.  Except for the identity the two columns are scaled by 0.5 - 2 and perturbed:
    not orthonormal, as refined poses are."""
    rng = np.random.RandomState(seed)
    out = []
    for T in lengths:
        x = np.zeros((T, J, 6))
        for j in range(J):
            kind = j % 4
            noise = expmap(rng.normal(scale=0.03, size=(T, 3)))
            if kind == 0:
                base = expmap(_unit(rng, 1) * rng.uniform(0, np.pi))[0]
                R = base[None] @ expmap(_unit(rng, 1) * (rng.uniform(0, 2 * np.pi) + rng.uniform(0.02, 0.08) * np.arange(T))[:, None]) @ noise
            elif kind == 1:
                ax = _unit(rng, 1) + 0.02 * np.cumsum(rng.normal(size=(T, 3)), 0)
                ax /= np.linalg.norm(ax, axis=1, keepdims=True)
                R = expmap(ax * (np.pi - rng.uniform(0, 1e-3, size=(T, 1))))
            elif kind == 2:
                x[:, j] = to_6d(np.eye(3))
                continue
            else:
                R = rot6d(sign_crossing(T, axis=_unit(rng, 1)[0])) @ noise
            x[:, j] = to_6d(R) * np.repeat(rng.uniform(0.5, 2.0, size=(T, 1, 2)), 3, 1).reshape(T, 6) + rng.normal(scale=0.02, size=(T, 6))
        out.append(x)
    return np.concatenate(out).astype(np.float32)


def table_case(seed):
    """(table (96,240) float32, order (70,) int32, run (70,) int32): the positions' records scattered over the rows by a non-monotone
    permutation; the 26 rows nobody lists are unrefined (all zero) and lie in between"""
    rng = np.random.RandomState(seed + 100)
    order = rng.permutation(N_ROWS)[:M].astype(np.int32)
    assert (np.diff(order) < 0).any() and (np.diff(order) > 0).any()
    x6d = trajectories(seed)
    table = np.zeros((N_ROWS, ROW), dtype=np.float32)
    table[order, 0:72] = rng.normal(size=(M, 72))                       # the axis-angle part: the kernels do not read it
    table[order, 72:216] = x6d.reshape(M, 144)
    table[order, 216:229] = rng.normal(size=(M, 13))
    table[order[5], 216], table[order[40], 227] = -0.0, -0.0             # a signed zero survives radius 0
    table[order, 229] = 1.0
    table[order, 230:237] = rng.uniform(size=(M, 7))
    return table, order, run_of_positions()


def positions_of(table, order):
    """(x6d (M,24,6), betas (M,10), cam (M,3)) float32 in position order"""
    rows = table[order]
    return rows[:, 72:216].reshape(-1, 24, 6), rows[:, 216:226], rows[:, 226:229]
