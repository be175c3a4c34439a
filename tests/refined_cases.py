"""Host restatement and cases of the refined-pose export (csrc/export.hip, refined.py): the log map R -> axis-angle as
include/jrr.h states it, the 6-D map (scripts/utils.py:190-204) and smplx batch_rodrigues, in numpy for a chosen dtype.

There is no reference implementation of the log map: the yardstick is float64.  The distance of the float32 evaluation of these
functions from their float64 evaluation, on a test's own inputs, is what the GPU is held to: `bound(d) = 3 d + 1e-7` (the margin
DESIGN section 3a uses for the crop kernel: the device's atan2f and the last bits of another evaluation order).
"""
import numpy as np

PI = np.pi
HALF_TURN_AXES = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 1, 1], [-1, 2, 0]], dtype=np.float64)
N_PLANTED = 1 + len(HALF_TURN_AXES)
NEAR_PI = 1e-3              # within this of pi, aa and aa - 2 pi axis denote (nearly) the same rotation: compare matrices


def bound(d):
    return 3.0 * float(d) + 1e-7


# ---- the restatement ------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """a * b + c rounded once for float32 operands (the product of two float32 is exact in float64); for float64 operands a plain
    product and sum -- the residuals the kernel keeps are then rounding noise at 1e-16, far below anything measured here"""
    if a.dtype == np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return a * b + c


def log_map(R, dtype=np.float64):
    """R (n,3,3) -> aa (n,3) in `dtype`, every operation rounded once in the order of csrc/export.hip rotmat_log"""
    R = np.asarray(R).astype(dtype).reshape(-1, 9)
    one, two, three = dtype(1), dtype(2), dtype(3)
    r = [R[:, k] for k in range(9)]
    r00, r11, r22 = r[0], r[4], r[8]
    with np.errstate(all='ignore'):
        tr = r00 + r11 + r22
        c0 = (tr >= r00) & (tr >= r11) & (tr >= r22)
        c1 = ~c0 & (r00 >= r11) & (r00 >= r22)
        c2 = ~c0 & ~c1 & (r11 >= r22)
        quats = [(one + tr, r[7] - r[5], r[2] - r[6], r[3] - r[1]),
                 (r[7] - r[5], one + r00 - r11 - r22, r[1] + r[3], r[2] + r[6]),
                 (r[2] - r[6], r[1] + r[3], one + r11 - r00 - r22, r[5] + r[7]),
                 (r[3] - r[1], r[2] + r[6], r[5] + r[7], one + r22 - r00 - r11)]
        w, x, y, z = (np.where(c0, quats[0][k], np.where(c1, quats[1][k], np.where(c2, quats[2][k], quats[3][k]))) for k in range(4))
        first = np.where(x != 0, x, np.where(y != 0, y, z))
        neg = (w < 0) | ((w == 0) & (first < 0))
        w, x, y, z = (np.where(neg, -v, v) for v in (w, x, y, z))
        xx, yy, zz = x * x, y * y, z * z
        t1 = xx + yy
        v1 = t1 - xx
        e1 = (xx - (t1 - v1)) + (yy - v1)
        t = t1 + zz
        v2 = t - t1
        e2 = (t1 - (t - v2)) + (zz - v2)
        lo = ((fma(x, x, -xx) + fma(y, y, -yy)) + fma(z, z, -zz)) + (e1 + e2)
        s = np.sqrt(t)
        q = s / w
        fs = (two / w) * (one - q * q / three)
        s_lo = (fma(-s, s, t) + lo) / (two * s)
        th = two * np.arctan2(s, w)
        f = th / s
        f_lo = (fma(-f, s, th) - f * s_lo) / s
        series = s <= dtype(1e-4) * w
        out = np.stack([np.where(series, v * fs, fma(v, f, v * f_lo)) for v in (x, y, z)], 1)
    assert out.dtype == dtype
    return out


def rot6d(x, dtype=np.float64):
    """(n,6) -> (n,3,3): columns b1, b2, b1 x b2 of the Gram-Schmidt of a1 = x[0::2], a2 = x[1::2] (csrc/rot6.h)"""
    x = np.asarray(x).astype(dtype).reshape(-1, 6)
    eps = dtype(1e-12)
    a1, a2 = x[:, 0::2], x[:, 1::2]
    b1 = a1 / np.maximum(np.sqrt((a1 * a1).sum(1)), eps)[:, None]
    u = a2 - (b1 * a2).sum(1)[:, None] * b1
    b2 = u / np.maximum(np.sqrt((u * u).sum(1)), eps)[:, None]
    b3 = np.cross(b1, b2)
    return np.stack([b1, b2, b3], 2)


def rodrigues(aa, dtype=np.float64, quirk=True):
    """smplx batch_rodrigues as k_rodrigues_fwd evaluates it (theta = |aa + 1e-8|, 1 - cos as 2 sin^2(theta / 2)); quirk=False: the
    exact exponential map (theta = |aa|, identity at 0)"""
    aa = np.asarray(aa).astype(dtype).reshape(-1, 3)
    e = aa + dtype(1e-8) if quirk else aa
    th = np.sqrt((e * e).sum(1))
    safe = np.where(th > 0, th, dtype(1))
    r = aa / safe[:, None]
    K = np.zeros((aa.shape[0], 3, 3), dtype=dtype)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -r[:, 2], r[:, 1], r[:, 2], -r[:, 0], -r[:, 1], r[:, 0]
    sh = np.sin(dtype(0.5) * th)
    out = np.eye(3, dtype=dtype)[None] + np.sin(th)[:, None, None] * K + (dtype(2) * sh * sh)[:, None, None] * (K @ K)
    assert out.dtype == dtype
    return out


def half_turn_expected():
    """the canonical vectors of the planted half-turns: pi * axis, the first non-zero component positive"""
    ax = HALF_TURN_AXES / np.linalg.norm(HALF_TURN_AXES, axis=1, keepdims=True)
    ax[5] = -ax[5]                                          # (-1, 2, 0) / sqrt 5 -> (+1.405, -2.810, 0)
    return PI * ax


# ---- cases ----------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def axis_angle_cases(n, seed):
    """(n,3) float64: [identity | six exact half-turns | angles pi - 10^u, u in [-8,-1] | angles 10^u, u in [-9,-1] | random axes with
    angles uniform in [0, pi]]; the first N_PLANTED rows are the planted ones, a quarter each of the rest for the two special ranges"""
    rng = np.random.RandomState(seed)
    m = n - N_PLANTED
    assert m >= 8
    n_pi, n_small = m // 4, m // 4
    ax = HALF_TURN_AXES / np.linalg.norm(HALF_TURN_AXES, axis=1, keepdims=True)
    parts = [np.zeros((1, 3)), PI * ax,
             _unit(rng, n_pi) * (PI - 10.0 ** rng.uniform(-8, -1, size=(n_pi, 1))),
             _unit(rng, n_small) * 10.0 ** rng.uniform(-9, -1, size=(n_small, 1)),
             _unit(rng, m - n_pi - n_small) * rng.uniform(0, PI, size=(m - n_pi - n_small, 1))]
    return np.concatenate(parts)


def planted_matrices():
    """float32 (N_PLANTED,3,3): the exact identity and the half-turns 2 n n^T - I (symmetric to the bit)"""
    ax = HALF_TURN_AXES / np.linalg.norm(HALF_TURN_AXES, axis=1, keepdims=True)
    H = 2.0 * ax[:, :, None] * ax[:, None, :] - np.eye(3)[None]
    return np.concatenate([np.eye(3)[None], H]).astype(np.float32)


def matrix_cases(n, seed):
    """float32 (n,3,3): axis_angle_cases through the exact exponential map in float64, rounded; the planted rows exact"""
    R = rodrigues(axis_angle_cases(n, seed), np.float64, quirk=False).astype(np.float32)
    R[:N_PLANTED] = planted_matrices()
    return R


def rot6d_cases(n, seed):
    """float32 (n,6): the first two columns of matrix_cases, each scaled by 0.5 - 2 and perturbed by 0.02 -- not orthonormal, as refined
    poses are"""
    rng = np.random.RandomState(seed + 1)
    R = rodrigues(axis_angle_cases(n, seed), np.float64, quirk=False)
    cols = R[:, :, :2] * rng.uniform(0.5, 2.0, size=(n, 1, 2)) + rng.normal(scale=0.02, size=(n, 3, 2))
    return cols.reshape(n, 6).astype(np.float32)


# ---- distances ------------------------------------------------------------------------------------------------------------
def distances(aa, aa64):
    """(vector distance over the rows whose float64 angle is farther than NEAR_PI from pi, matrix distance over ALL rows): max-abs, the
    matrices by the exact exponential map in float64.  NaN anywhere makes the distance NaN (and every assertion on it false)."""
    aa, aa64 = np.asarray(aa, dtype=np.float64).reshape(-1, 3), np.asarray(aa64, dtype=np.float64).reshape(-1, 3)
    far = np.linalg.norm(aa64, axis=1) < PI - NEAR_PI
    d_vec = np.abs(aa[far] - aa64[far]).max() if far.any() else 0.0
    d_mat = np.abs(rodrigues(aa, np.float64, quirk=False) - rodrigues(aa64, np.float64, quirk=False)).max()
    return float(d_vec), float(d_mat)


def yardsticks(R32):
    """for float32 matrices: (aa64 = float64 log, d_vec, d_mat of the float32 log from it, round-trip distance of the float32
    restatement: batch_rodrigues in float32 of the float32 log, from R itself)"""
    aa64, aa32 = log_map(R32, np.float64), log_map(R32, np.float32)
    d_vec, d_mat = distances(aa32, aa64)
    d_rt = float(np.abs(rodrigues(aa32, np.float32).astype(np.float64) - np.asarray(R32, dtype=np.float64).reshape(-1, 3, 3)).max())
    return aa64, d_vec, d_mat, d_rt


def yardsticks_6d(x32):
    """end to end from 6-D input: (aa64 = float64 Gram-Schmidt + log, d_vec, d_mat of the all-float32 evaluation from it)"""
    aa64 = log_map(rot6d(x32, np.float64), np.float64)
    d_vec, d_mat = distances(log_map(rot6d(x32, np.float32), np.float32), aa64)
    return aa64, d_vec, d_mat


# ---- the table on the host -------------------------------------------------------------------------------------------------
def host_rows(x6d, betas, cam, extra=None):
    """(B,240) float32: the rows k_pose_export writes, axis-angle by the float32 restatement"""
    B = x6d.shape[0]
    row = np.zeros((B, 240), dtype=np.float32)
    row[:, 0:72] = log_map(rot6d(x6d.reshape(-1, 6), np.float32), np.float32).reshape(B, 72)
    row[:, 72:216] = x6d.reshape(B, 144)
    row[:, 216:226], row[:, 226:229], row[:, 229] = betas, cam, 1.0
    if extra is not None:
        row[:, 230:230 + extra.shape[1]] = extra
    return row


def export_case(B, seed):
    rng = np.random.RandomState(seed)
    return (rot6d_cases(B * 24, seed).reshape(B, 24, 6), rng.normal(size=(B, 10)).astype(np.float32),
            rng.normal(size=(B, 3)).astype(np.float32))
