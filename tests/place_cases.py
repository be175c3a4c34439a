"""Inputs and the float64 host restatement of `--place_refined` (include/jrr.h: jrr_place_translation, jrr_project_points,
jrr_place_accumulate), shared by tests/test_place.py and tests/test_gpu_place.py.

The restatement is written from the header's formulas alone, vectorised over the poses: float64 on the float32 inputs, every
operation a numpy ufunc of its own (rounded once, nothing fused) in the header's order, sums over the joints ascending.  The reference
has no runnable counterpart (scripts/create_smpl_gt.py keeps the step commented out), so there is no golden.

Cases (all seeded): 17 points spread 0.25 / 0.45 / 0.15 m about a point near the origin, planted translations with depth 2.5 .. 7 m
and lateral offsets up to 1.5 m, fx != fy in 1100 .. 1200, principal point 480 .. 540; even cases carry exact pixels (projected in
float64, rounded to float32), odd cases 5 px Gaussian noise; every third case has 5 random weights set to zero, every fifth non-unit
weights in 0.25 .. 4.  The four refusals: one taking-part joint, a NaN pixel (bit 0), all joints coincident (bit 1; built from numbers
for which every operation of the factorisation is exact, so that the last pivot is exactly 0 on any IEEE machine), pixels of a body
planted BEHIND the camera (bit 2: the linear start finds that translation).
"""
import numpy as np

F, F64 = np.float32, np.float64
NJ = 17
BIT_FEW, BIT_PIVOT, BIT_BEHIND, BIT_STEP = 1, 2, 4, 8
BAD_BITS = 7
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-7, 1e7
# the table row (include/jrr.h, JRR_PLACE_ACC_*)
ROW, TRAILER = 55, 2
COUNT, BAD, STEP_PIVOT, SUM_TZ, JOINTS, SUM_ERR_LIN, SUM_ERR = 0, 1, 2, 3, 4, 21, 38
ERR_CAP = F(1.0e3)
GPU_BATCHES = (1, 2, 63, 64, 65, 257, 1000)
GPU_ITERS = (0, 1, 10)
GPU_POOL = 1000
REFUSALS = {'one_joint': BIT_FEW, 'nan_pixel': BIT_FEW, 'coincident': BIT_PIVOT, 'behind': BIT_BEHIND}
REFUSAL_AT = {'one_joint': 1, 'nan_pixel': 40, 'coincident': 64, 'behind': 200}      # their places in the pool; again at 600 + k
PROJECT_POINTS = (1, 17, 6890)


def project64(points, trans, K):
    """float64 pinhole projection of points (B,N,3) + trans (B,3) under K (B,3,3): (uv (B,N,2), depth (B,N)), no Z test"""
    P = np.asarray(points, F64) + np.asarray(trans, F64)[:, None]
    K = np.asarray(K, F64)
    with np.errstate(all='ignore'):
        u = K[:, None, 0, 0] * P[..., 0] / P[..., 2] + K[:, None, 0, 2]
        v = K[:, None, 1, 1] * P[..., 1] / P[..., 2] + K[:, None, 1, 2]
    return np.stack([u, v], -1), P[..., 2]


def cameras(n, rng):
    K = np.zeros((n, 3, 3), F)
    K[:, 0, 0], K[:, 1, 1] = rng.uniform(1100, 1150, n), rng.uniform(1150, 1200, n)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = rng.uniform(480, 540, n), rng.uniform(480, 540, n), 1
    K[:, 0, 1], K[:, 1, 0], K[:, 2, 0] = 7.0, -3.0, 0.5                              # entries nobody may read
    return K


def bodies(n, rng):
    return (rng.normal(size=(n, NJ, 3)) * [0.25, 0.45, 0.15] + rng.uniform(-0.2, 0.2, size=(n, 1, 3))).astype(F)


def regular_cases(n, seed=0):
    """(joints (n,17,3) f32, j2d (n,17,2) f32, K (n,3,3) f32, weight (n,17) f32, planted (n,3) f64, exact (n,) bool)"""
    rng = np.random.RandomState(seed)
    joints, K = bodies(n, rng), cameras(n, rng)
    planted = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2.5, 7.0, n)], 1)
    uv, depth = project64(joints, planted, K)
    assert (depth > 1.0).all()
    exact = np.arange(n) % 2 == 0
    noise = rng.normal(0, 5.0, size=uv.shape)
    j2d = np.where(exact[:, None, None], uv, uv + noise).astype(F)
    weight = np.ones((n, NJ), F)
    for i in range(n):
        draw = rng.uniform(0.25, 4.0, NJ), rng.permutation(NJ)[:5]                   # drawn for every case: a case does not depend on n
        if i % 5 == 4:
            weight[i] = draw[0]
        if i % 3 == 2:
            weight[i, draw[1]] = 0
    return joints, j2d, K, weight, planted, exact


def refusal_case(name, seed=7):
    """one pose (joints (17,3), j2d (17,2), K (3,3), weight (17,)) for which the restatement reports REFUSALS[name]"""
    rng = np.random.RandomState(seed)
    joints, K = bodies(1, rng)[0], cameras(1, rng)[0]
    planted = np.array([0.3, -0.2, 4.0])
    j2d = project64(joints[None], planted[None], K[None])[0][0].astype(F)
    weight = np.ones(NJ, F)
    if name == 'one_joint':
        weight[:] = 0
        weight[3] = 1
        weight[9], weight[12] = np.nan, -1.0                                         # neither takes part
    elif name == 'nan_pixel':
        j2d[6, 1] = np.nan
    elif name == 'coincident':
        # S + t = (0.5, -0.25, 4) for every joint; fx = 1152, fy = 1120, c = (512, 500): a = 144, b = -70, l20 = -1/8, l21 = 1/16 and
        # d2 = 17 (a^2 + b^2) - 17 a^2 - 17 b^2 = 0 with every product and quotient exact
        joints = np.tile(F([0.25, -0.5, 0.5]), (NJ, 1))
        K = np.zeros((3, 3), F)
        K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[2, 2] = 1152, 1120, 512, 500, 1
        j2d = np.tile(F([512 + 144, 500 - 70]), (NJ, 1))
    elif name == 'behind':
        j2d = project64(joints[None], np.array([[0.3, -0.2, -5.0]]), K[None])[0][0].astype(F)
    else:
        raise KeyError(name)
    return joints, j2d, K, weight


def gpu_pool():
    """(joints, j2d, K, weight, planted, regular (1000,) bool): regular_cases(1000) with the four refusals at REFUSAL_AT and at 600 + k"""
    joints, j2d, K, weight, planted, exact = regular_cases(GPU_POOL, seed=11)
    regular = np.ones(GPU_POOL, bool)
    for k, name in enumerate(REFUSALS):
        for at in (REFUSAL_AT[name], 600 + k):
            joints[at], j2d[at], K[at], weight[at] = refusal_case(name)
            regular[at], planted[at] = False, np.nan
    return joints, j2d, K, weight, planted, regular


# ---- jrr_place_translation in float64 ----------------------------------------------------------------------------------------
def _solve(a00, a01, a02, a11, a12, a22, y0, y1, y2):
    with np.errstate(all='ignore'):
        d0 = a00
        l10, l20 = a01 / d0, a02 / d0
        d1 = a11 - l10 * a01
        m = a12 - l20 * a01
        l21 = m / d1
        d2 = (a22 - l20 * a02) - l21 * m
        ok = (d0 > 0) & (d1 > 0) & (d2 > 0)
        z0 = y0
        z1 = y1 - l10 * z0
        z2 = (y2 - l20 * z0) - l21 * z1
        x2 = z2 / d2
        x1 = z1 / d1 - l21 * x2
        x0 = (z0 / d0 - l10 * x1) - l20 * x2
    return ok, x0, x1, x2


class _Pose:
    def __init__(self, joints, j2d, K, weight):
        self.S, self.uv, K = np.asarray(joints, F).astype(F64), np.asarray(j2d, F).astype(F64), np.asarray(K, F)
        B = self.S.shape[0]
        self.fx, self.fy, self.cx, self.cy = (K[:, r, c].astype(F64) for r, c in ((0, 0), (1, 1), (0, 2), (1, 2)))
        w = np.ones((B, NJ), F) if weight is None else np.asarray(weight, F)
        with np.errstate(invalid='ignore'):
            self.part = np.isfinite(w) & (w > 0)
        self.w = np.where(self.part, w, 0).astype(F64)
        self.finite = (np.isfinite(self.S).all((1, 2)) & np.isfinite(self.uv).all((1, 2)) & np.isfinite(self.fx) & np.isfinite(self.fy) &
                       np.isfinite(self.cx) & np.isfinite(self.cy))

    def cost(self, t0, t1, t2):
        """(cost (B,), front (B,), err (B,17) float32) at t"""
        B = self.S.shape[0]
        c, front, err = np.zeros(B), np.ones(B, bool), np.zeros((B, NJ), F)
        with np.errstate(all='ignore'):
            for j in range(NJ):
                X, Y, Z = self.S[:, j, 0] + t0, self.S[:, j, 1] + t1, self.S[:, j, 2] + t2
                ru = ((self.fx * X) / Z + self.cx) - self.uv[:, j, 0]
                rv = ((self.fy * Y) / Z + self.cy) - self.uv[:, j, 1]
                e2 = ru * ru + rv * rv
                err[:, j] = np.sqrt(e2).astype(F)
                c = c + np.where(self.part[:, j], self.w[:, j] * e2, 0.0)
                front &= np.where(self.part[:, j], Z > 0, True)
        return c, front, err

    def linear(self):
        B = self.S.shape[0]
        a00, a02, a11, a12, a22, y0, y1, y2 = (np.zeros(B) for _ in range(8))
        with np.errstate(all='ignore'):
            for j in range(NJ):
                p, w = self.part[:, j], self.w[:, j]
                X, Y, Z = self.S[:, j, 0], self.S[:, j, 1], self.S[:, j, 2]
                a, b = self.uv[:, j, 0] - self.cx, self.uv[:, j, 1] - self.cy
                r1, r2 = a * Z - self.fx * X, b * Z - self.fy * Y
                z = lambda v: np.where(p, v, 0.0)
                a00 = a00 + z(w * self.fx * self.fx)
                a02 = a02 - z(w * self.fx * a)
                a11 = a11 + z(w * self.fy * self.fy)
                a12 = a12 - z(w * self.fy * b)
                a22 = a22 + z(w * (a * a + b * b))
                y0 = y0 + z(w * self.fx * r1)
                y1 = y1 + z(w * self.fy * r2)
                y2 = y2 - z(w * (a * r1 + b * r2))
        return _solve(a00, np.zeros(B), a02, a11, a12, a22, y0, y1, y2)

    def step_system(self, t0, t1, t2):
        B = self.S.shape[0]
        h00, h02, h11, h12, h22, g0, g1, g2 = (np.zeros(B) for _ in range(8))
        with np.errstate(all='ignore'):
            for j in range(NJ):
                p, w = self.part[:, j], self.w[:, j]
                X, Y, Z = self.S[:, j, 0] + t0, self.S[:, j, 1] + t1, self.S[:, j, 2] + t2
                ru = ((self.fx * X) / Z + self.cx) - self.uv[:, j, 0]
                rv = ((self.fy * Y) / Z + self.cy) - self.uv[:, j, 1]
                q = 1.0 / Z
                ju0, jv1 = self.fx * q, self.fy * q
                ju2, jv2 = -(ju0 * X) * q, -(jv1 * Y) * q
                z = lambda v: np.where(p, v, 0.0)
                h00 = h00 + z(w * ju0 * ju0)
                h02 = h02 + z(w * ju0 * ju2)
                h11 = h11 + z(w * jv1 * jv1)
                h12 = h12 + z(w * jv1 * jv2)
                h22 = h22 + z(w * (ju2 * ju2 + jv2 * jv2))
                g0 = g0 + z(w * ju0 * ru)
                g1 = g1 + z(w * jv1 * rv)
                g2 = g2 + z(w * (ju2 * ru + jv2 * rv))
        return h00, h02, h11, h12, h22, g0, g1, g2


def place(joints, j2d, K, weight=None, n_iters=10):
    """the float64 restatement: dict with trans (B,3) f64, trans_linear (B,3) f64, err_lin / err (B,17) f32, status (B,) int32, costs
    (n_iters + 1, B) -- the carried cost at the start and after every step --, accepted (n_iters, B) bool"""
    p = _Pose(joints, j2d, K, weight)
    B = p.S.shape[0]
    status = np.where((p.part.sum(1) < 2) | ~p.finite, BIT_FEW, 0).astype(np.int32)
    ok, t0, t1, t2 = p.linear()
    status = np.where((status == 0) & ~ok, BIT_PIVOT, status)
    c, front, err_lin = p.cost(t0, t1, t2)
    status = np.where((status == 0) & ~front, BIT_BEHIND, status).astype(np.int32)
    t_lin = np.stack([t0, t1, t2], 1)
    live = status == 0
    lam = np.full(B, LAMBDA0)
    costs, accepted = [c.copy()], []
    for _ in range(int(n_iters)):
        h00, h02, h11, h12, h22, g0, g1, g2 = p.step_system(t0, t1, t2)
        ok, d0, d1, d2 = _solve(h00 + lam * h00, np.zeros(B), h02, h11 + lam * h11, h12, h22 + lam * h22, -g0, -g1, -g2)
        n0, n1, n2 = t0 + d0, t1 + d1, t2 + d2
        cn, fr, _ = p.cost(n0, n1, n2)
        with np.errstate(invalid='ignore'):
            accept = live & ok & (cn < c) & fr
        status = np.where(live & ~ok, status | BIT_STEP, status).astype(np.int32)
        t0, t1, t2, c = np.where(accept, n0, t0), np.where(accept, n1, t1), np.where(accept, n2, t2), np.where(accept, cn, c)
        lam = np.where(accept, np.maximum(lam / 10.0, LAMBDA_MIN), np.minimum(10.0 * lam, LAMBDA_MAX))
        costs.append(c.copy())
        accepted.append(accept)
    _, _, err = p.cost(t0, t1, t2)
    trans = np.stack([t0, t1, t2], 1)
    bad = (status & BAD_BITS) != 0
    trans[bad], t_lin[bad], err[bad], err_lin[bad] = np.nan, np.nan, np.nan, np.nan
    return {'trans': trans, 'trans_linear': t_lin, 'err_lin': err_lin, 'err': err, 'status': status, 'costs': np.array(costs),
            'accepted': np.array(accepted).reshape(int(n_iters), B)}


def cost64(joints, j2d, K, weight, trans):
    """c(t) of the header for poses at translations `trans` (B,3), float64"""
    t = np.asarray(trans, F64)
    return _Pose(joints, j2d, K, weight).cost(t[:, 0], t[:, 1], t[:, 2])[0]


# ---- jrr_project_points ---------------------------------------------------------------------------------------------------------
def project_case(n_points, seed=5, B=3):
    """(points (B,N,3) f32, trans (B,3) f64, K (B,3,3) f32): bodies in front of the camera, but the points of pose 1 straddle Z + tz = 0
    (for N = 1: pose 1's only point lies behind it)"""
    rng = np.random.RandomState(seed + n_points)
    points = (rng.normal(size=(B, n_points, 3)) * [0.25, 0.45, 0.15]).astype(F)
    trans = np.stack([rng.uniform(-1.5, 1.5, B), rng.uniform(-1.5, 1.5, B), rng.uniform(2.5, 7.0, B)], 1)
    trans[1, 2] = -0.01 if n_points > 1 else -3.0
    points[1, 0, 2] = F(0.01)                                                        # Z + tz == 0 exactly in float32: not in front
    return points, trans, cameras(B, rng)


def project_reference(points, trans, K):
    """(uv (B,N,2) f64 with NaN where Z + tz <= 0, depth (B,N) f64, bound (B,N,2)): float64 arithmetic on the float32 inputs, trans
    rounded to float32 once as the header says; bound = 16 * 2^-24 * (|f X / Z| + |c|)"""
    t32 = np.asarray(trans, F64).astype(F)
    uv, depth = project64(points, t32, K)
    K = np.asarray(K, F64)
    c = np.stack([K[:, 0, 2], K[:, 1, 2]], -1)[:, None]
    bound = 16 * 2.0 ** -24 * (np.abs(uv - c) + np.abs(c))
    behind = ~(depth > 0)
    uv[behind] = np.nan
    return uv, depth, bound


# ---- jrr_place_accumulate ---------------------------------------------------------------------------------------------------
def fixed24(v):
    """llrintf(v * 2^24) of float32 values: the product is exact in float32 below the cap"""
    return np.rint((np.asarray(v, F) * F(16777216.0)).astype(F64)).astype(np.int64)


def accumulate(trans, err_lin, err, weight, status, group, n_groups):
    """the int64 table (n_groups * 55 + 2,) of the poses the kernel wrote, in Python integers / numpy int64"""
    B = err.shape[0]
    table = np.zeros(n_groups * ROW + TRAILER, np.int64)
    w = np.ones((B, NJ), F) if weight is None else np.asarray(weight, F)
    with np.errstate(invalid='ignore'):
        part = np.isfinite(w) & (w > 0)
    group = np.zeros(B, np.int32) if group is None else group
    for b in range(B):
        g = int(group[b])
        if g < 0:
            table[n_groups * ROW] += 1
            continue
        if g >= n_groups:
            table[n_groups * ROW + 1] += 1
            continue
        row = table[g * ROW:(g + 1) * ROW]
        tz = F(trans[b, 2])
        with np.errstate(invalid='ignore'):
            good = not (int(status[b]) & BAD_BITS) and bool(np.abs(tz) < ERR_CAP) and bool((err[b][part[b]] < ERR_CAP).all())
            if err_lin is not None:
                good = good and bool((err_lin[b][part[b]] < ERR_CAP).all())
        if not good:
            row[BAD] += 1
            continue
        row[COUNT] += 1
        row[STEP_PIVOT] += 1 if int(status[b]) & BIT_STEP else 0
        row[SUM_TZ] += fixed24(tz)
        row[JOINTS:JOINTS + NJ] += part[b]
        if err_lin is not None:
            row[SUM_ERR_LIN:SUM_ERR_LIN + NJ] += np.where(part[b], fixed24(np.where(part[b], err_lin[b], 0)), 0)
        row[SUM_ERR:SUM_ERR + NJ] += np.where(part[b], fixed24(np.where(part[b], err[b], 0)), 0)
    return table
