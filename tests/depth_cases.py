"""Host restatement and seeded inputs of the depth section of the regressor report (tests/test_joint_depth.py,
tests/test_gpu_joint_depth.py).

Written from include/jrr.h: the seven closest-point regions and the solid-angle formula of jrr_point_mesh_depth, the table layout
JRR_DEPTH_ACC_* and the arithmetic of jrr_depth_accumulate.  `dtype` float32 follows the kernel (each Omega in float32, their sum in
float64); float64 is the yardstick.  The kernel may fuse products into sums, numpy does not: the distance and the winding number are
compared within `bound(d)`, d being the float32 restatement's own distance from the float64 one on the same inputs; the accumulator
is integers and compared word for word.  Inputs are regenerated from seeds, never stored."""
import functools
import importlib

import numpy as np

from conftest import PKG_NAME

F32, F64 = np.float32, np.float64
NJ = 17
ROW, TRAILER, COLS, BINS = 4290, 2, 64, 64
COUNT, BAD, OUTSIDE, UNSURE, SUM, HIST = 0, 1, 2, 66, 130, 194
REGIONS = ('a', 'b', 'ab', 'c', 'ac', 'bc', 'interior')
MAX_POINTS = 64


def bound(d):
    """the project's margin over the float32 restatement's own error d"""
    return 3.0 * float(d) + 1e-7


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


# ---- the restatement -------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def pair_terms(verts, faces, points, dtype=F64):
    """one pose: verts (V,3), faces (F,3), points (P,3) -> per (point, face) the squared distance (P,F) (NaN where the face has no
    area; +inf for a face with an index outside [0, V)), the region index into REGIONS (P,F) and the solid angle Omega (P,F) in `dtype`
    (0 for a face that is skipped)"""
    v = np.asarray(verts).astype(dtype)
    p = np.asarray(points).astype(dtype)
    f = np.asarray(faces).astype(np.int64)
    ok = ((f >= 0) & (f < v.shape[0])).all(axis=1)
    fs = np.where(ok[:, None], f, 0)
    a, b, c = v[fs[:, 0]][None], v[fs[:, 1]][None], v[fs[:, 2]][None]
    P = p[:, None, :]
    with np.errstate(all='ignore'):
        ab, ac = b - a, c - a
        A, B, C = a - P, b - P, c - P
        d1, d2, d3, d4, d5, d6 = -_dot(ab, A), -_dot(ac, A), -_dot(ab, B), -_dot(ac, B), -_dot(ab, C), -_dot(ac, C)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        d43, d56 = d4 - d3, d5 - d6
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d43 >= 0) & (d56 >= 0)]
        region = np.full(d1.shape, 6, dtype=np.int64)
        for k in range(5, -1, -1):
            region = np.where(conds[k], k, region)
        one = dtype(1)
        den = np.select([region == 2, region == 4, region == 5], [d1 - d3, d2 - d6, d43 + d56], va + vb + vc)
        r = one / den
        vv = np.select([region == 2, region == 4, region == 5], [d1, np.zeros_like(r), d56], vb) * r
        uu = np.select([region == 2, region == 4, region == 5], [np.zeros_like(r), d2, d43], vc) * r
        e = A + vv[..., None] * ab + uu[..., None] * ac
        dl = np.where((region == 0)[..., None], A, np.where((region == 1)[..., None], B, np.where((region == 3)[..., None], C, e)))
        d2f = _dot(dl, dl)
        la, lb, lc = np.sqrt(_dot(A, A)), np.sqrt(_dot(B, B)), np.sqrt(_dot(C, C))
        num = _dot(A, _cross(B, C))
        dn = la * lb * lc + _dot(A, B) * lc + _dot(B, C) * la + _dot(C, A) * lb
        omega = dtype(2) * np.arctan2(num, dn)
    d2f = np.where(ok[None, :], d2f, np.inf)
    omega = np.where(ok[None, :], omega, 0).astype(dtype)
    return d2f, region, omega


def depth(verts, faces, points, dtype=F64):
    """one pose -> dict: dist (P,), wind (P,), face (P,) the smallest index among the equal computed minima, region (P,) of that face,
    all (P,F) the distance to every face (NaN / inf as pair_terms), status (bit 0: a face was skipped)"""
    d2f, region, omega = pair_terms(verts, faces, points, dtype)
    key = np.where(np.isnan(d2f), np.inf, d2f)
    face = np.argmin(key, axis=1)                                    # the first of equal values
    best = key[np.arange(key.shape[0]), face]
    wind = omega.astype(F64).sum(axis=1) / (4.0 * np.pi)
    f = np.asarray(faces)
    status = int(((f < 0) | (f >= np.asarray(verts).shape[0])).any())
    poisoned = ~np.isfinite(np.asarray(points, dtype=F64)).all(axis=1) | (not np.isfinite(np.asarray(verts, dtype=F64)).all())
    with np.errstate(all='ignore'):
        out = {'dist': np.where(poisoned, np.nan, np.sqrt(best)).astype(dtype), 'wind': np.where(poisoned, np.nan, wind).astype(dtype),
               'face': np.where(poisoned | ~np.isfinite(best), -1, face), 'region': region[np.arange(key.shape[0]), face],
               'all': np.sqrt(d2f), 'status': status}
    return out


def depth_batch(verts, faces, points, dtype=F64):
    """verts (B,V,3), points (B,P,3): the per-pose results stacked"""
    rows = [depth(verts[b], faces, points[b], dtype) for b in range(verts.shape[0])]
    out = {k: np.stack([r[k] for r in rows]) for k in ('dist', 'wind', 'face', 'region', 'all')}
    out['status'] = int(any(r['status'] for r in rows))
    return out


def inside(wind):
    with np.errstate(invalid='ignore'):
        return np.abs(np.asarray(wind, dtype=F32)) > F32(0.5)


# ---- the accumulator -------------------------------------------------------------------------------------------------------
def accumulate(dist, wind, group, n_groups, table=None):
    """ADD to `table` (int64, n_groups * 4290 + 2; None = zeros) what jrr_depth_accumulate adds, in exact integers; every float32
    operation rounded once, in the order the header writes them"""
    dist, wind = np.asarray(dist, dtype=F32), np.asarray(wind, dtype=F32)
    B, P = dist.shape
    t = np.zeros(n_groups * ROW + TRAILER, dtype=np.int64) if table is None else table
    for b in range(B):
        g = 0 if group is None else int(group[b])
        if g < 0:
            t[n_groups * ROW] += 1
            continue
        if g >= n_groups:
            t[n_groups * ROW + 1] += 1
            continue
        row = t[g * ROW:(g + 1) * ROW]
        d, w = dist[b], wind[b]
        if not (np.isfinite(d).all() and np.isfinite(w).all() and (d < F32(1.0e3)).all()):
            row[BAD] += 1
            continue
        row[COUNT] += 1
        aw = np.abs(w)
        ins = aw > F32(0.5)
        dep = np.where(ins, d, -d).astype(F32)
        row[OUTSIDE:OUTSIDE + P] += (~ins).astype(np.int64)
        row[UNSURE:UNSURE + P] += (np.abs((aw - np.rint(aw)).astype(F32)) > F32(0.1)).astype(np.int64)
        row[SUM:SUM + P] += np.rint((dep * F32(16777216.0)).astype(F32).astype(F64)).astype(np.int64)
        bins = np.clip(np.floor(((dep + F32(0.064)).astype(F32) * F32(250.0)).astype(F32)).astype(np.int64), 0, BINS - 1)
        for k in range(P):
            row[HIST + k * BINS + bins[k]] += 1
    return t


# ---- meshes ------------------------------------------------------------------------------------------------------------------
def _relabel(faces):
    """face k starts at its corner k mod 3: the orientation stays, which corner is `a` varies -- so every region label occurs"""
    return np.stack([np.roll(f, -(k % 3)) for k, f in enumerate(faces)]).astype(np.int32)


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=F64)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    return v, f


def cube():
    v = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], dtype=F64)     # index 4 x + 2 y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]                  # outward
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])
    return v, f


def sphere(levels):
    """the octahedron subdivided `levels` times onto the unit sphere: 4^levels * 8 faces"""
    v, f = octahedron()
    v = [tuple(x) for x in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = (np.array(v[i]) + np.array(v[j])) / 2
                v.append(tuple(x / np.linalg.norm(x)))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = np.array(nf)
    return np.array(v, dtype=F64), f


def is_closed(faces):
    """every directed edge occurs once and its reverse once"""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    fwd = e[:, 0] * (1 << 32) + e[:, 1]
    rev = e[:, 1] * (1 << 32) + e[:, 0]
    return np.unique(fwd).size == fwd.size and np.array_equal(np.sort(fwd), np.sort(rev))


def _rotation(rs):
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def _convex_points(v, f, rs):
    """64 points around a convex mesh that contains the origin: above and below face centres, beyond edge midpoints, beyond corners,
    and deep inside"""
    f = np.asarray(f)
    pts = []
    order = np.resize(rs.permutation(f.shape[0]), 10)                 # the octahedron has 8 faces: two are taken twice
    for k in order[:10]:
        c = v[f[k]].mean(0)
        n = np.cross(v[f[k, 1]] - v[f[k, 0]], v[f[k, 2]] - v[f[k, 0]])
        n /= np.linalg.norm(n)
        pts += [c + 0.05 * n, c - 0.05 * n, c + 0.3 * n]
    for k in order[:9]:
        for i in range(3):
            mid = (v[f[k, i]] + v[f[k, (i + 1) % 3]]) / 2
            pts.append(mid * (1.0 + 0.2 / np.linalg.norm(mid)))       # 0.2 beyond the edge midpoint, away from the centre
    for i in rs.permutation(v.shape[0])[:5]:
        pts.append(v[i] * (1.0 + 0.25 / np.linalg.norm(v[i])))      # 0.25 beyond a corner
    pts += [np.zeros(3), np.array([0.1, -0.05, 0.02])]
    pts = np.array(pts)
    assert pts.shape[0] == MAX_POINTS, pts.shape
    return pts


@functools.lru_cache(maxsize=None)
def convex_case(name):
    """(verts (5,V,3) f32, faces (F,3) i32, points (5,64,3) f32): pose 0 the mesh itself, poses 1..4 rigidly moved copies"""
    v, f = {'octahedron': octahedron, 'cube': cube, 'sphere2': lambda: sphere(2), 'sphere3': lambda: sphere(3)}[name]()
    rs = np.random.RandomState({'octahedron': 11, 'cube': 12, 'sphere2': 13, 'sphere3': 14}[name])
    pts = _convex_points(v, f, rs)
    V, P = [v], [pts]
    for _ in range(4):
        R, t = _rotation(rs), rs.uniform(-0.5, 0.5, size=3)
        V.append(v @ R.T + t)
        P.append(pts @ R.T + t)
    return np.stack(V).astype(F32), _relabel(f), np.stack(P).astype(F32)


@functools.lru_cache(maxsize=None)
def body_case():
    """(verts (3,6890,3) f32, faces (13776,3) i32, points (3,64,3) f32): the synthetic body's template and two rigidly moved copies
    with 0.5 mm of vertex noise; columns 0..16 the shipped regressor's joints on those vertices (inside), 17..33 the joints shifted by
    0.5 m along x, 34..50 along z, 51..63 the first 13 shifted down and back (outside, but for the few that land in another limb)"""
    sm, rr = _mod('smpl_model'), _mod('regressor_report')
    model = sm.synthetic_smpl()
    vt, faces = np.asarray(model['v_template'], dtype=F64), np.asarray(model['faces']).astype(np.int32)
    Jn = rr.normalised(sm.default_h36m_regressor())
    rs = np.random.RandomState(22)      # seed 21 leaves a joint 0.84 mm under the noisy skin: below the 1 mm the inside flags need
    V = [vt]
    for _ in range(2):
        R, t = _rotation(rs), rs.uniform(-0.3, 0.3, size=3)
        V.append(vt @ R.T + t + rs.normal(scale=0.0005, size=vt.shape))
    V = np.stack(V).astype(F32)
    P = []
    for b in range(3):
        j = Jn @ V[b].astype(F64)
        P.append(np.concatenate([j, j + [0.5, 0, 0], j + [0, 0, 0.5], j[:13] + [0, -0.5, -0.3]]))
    return V, faces, np.stack(P).astype(F32)


CONVEX = ('octahedron', 'cube', 'sphere2', 'sphere3')


def case(name):
    return body_case() if name == 'body' else convex_case(name)


@functools.lru_cache(maxsize=None)
def reference(name, dtype_name='f64'):
    """the restatement on the whole case (all poses, 64 points), computed once and shared; callers slice and do not write"""
    v, f, p = case(name)
    out = depth_batch(v, f, p, F64 if dtype_name == 'f64' else F32)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def driver_case():
    """the inputs of the driver tests: 6 meshes of the synthetic body (rigidly moved, 0.5 mm of vertex noise), the shipped regressor
    J, a retrained one J2 whose R_Wrist row keeps two vertices only -- 5068 and 1204, half each: their midpoint lies about 10 mm
    OUTSIDE the skin, the hull of the body not being the body -- and as ground truth (mm) the joints of a third, mildly different
    regressor; group ids.  -> dict(J, J2, verts, gt_mm, ids, faces).  Mesh seed 43: seeds 41 and 42 leave a point 0.75 / 0.94 mm
    from the surface, below the 1 mm the inside flags need."""
    sm = _mod('smpl_model')
    model = sm.synthetic_smpl()
    vt, faces = np.asarray(model['v_template'], dtype=F64), np.asarray(model['faces']).astype(np.int32)
    J = sm.default_h36m_regressor()
    J2 = (J * (1 + 0.5 * np.random.RandomState(5).rand(*J.shape))).astype(F32)
    J2[16] = 0
    J2[16, 5068] = J2[16, 1204] = 0.5
    J3 = (J * (1 + 0.2 * np.random.RandomState(6).rand(*J.shape))).astype(F32)
    rs = np.random.RandomState(43)
    V = np.stack([vt @ _rotation(rs).T + rs.uniform(-0.3, 0.3, size=3) + rs.normal(scale=0.0005, size=vt.shape) for _ in range(6)]).astype(F32)
    gt = (_mod('regressor_report').normalised(J3) @ V.astype(F64) * 1000.0).astype(F32)
    return {'J': J, 'J2': J2, 'verts': V, 'gt_mm': gt, 'ids': np.array([0, 1, 0, 1, 1, 0], dtype=np.int32), 'faces': faces, 'model': model}


def driver_points(joints_a, joints_b, gt_mm):
    """the 51 points per pose of the report: the joints of A, of B, and the ground truth, pelvis-centred, placed at A's pelvis"""
    gt = np.asarray(gt_mm, dtype=F64) / 1000.0
    ja = np.asarray(joints_a, dtype=F64)
    return np.concatenate([ja, np.asarray(joints_b, dtype=F64), gt - gt[:, :1] + ja[:, :1]], axis=1).astype(F32)


def driver_points_host():
    """driver_points with both regressors applied in float64 on the host (the device's float32 product moves a point by ~1e-7 m)"""
    c, rr = driver_case(), _mod('regressor_report')
    V = c['verts'].astype(F64)
    return driver_points(rr.normalised(c['J']) @ V, rr.normalised(c['J2']) @ V, c['gt_mm'])


def check_inside_conditions(r64):
    """the conditions on every point whose inside flag a test compares exactly: at least 1 mm from the surface, the winding number
    within 0.1 of an integer"""
    assert (r64['dist'] >= 1e-3).all(), float(r64['dist'].min())
    assert (np.abs(np.abs(r64['wind']) - 0.5) >= 0.4).all()


def hand_made_table(n_groups=2):
    """a table whose derived numbers are known: group 0 has 4 poses, group 1 none"""
    t = np.zeros(n_groups * ROW + TRAILER, dtype=np.int64)
    t[COUNT], t[BAD] = 4, 1
    t[OUTSIDE + 17 + 3] = 1                                  # retrained, joint 3: outside in one pose of four
    t[UNSURE + 34 + 5] = 2                                   # ground truth, joint 5: unsure in two
    t[SUM + 0] = 4 * int(0.010 * (1 << 24))                  # initial, joint 0: mean 10 mm (to the fixed-point unit)
    t[SUM + 17 + 3] = int(-0.002 * (1 << 24)) * 4
    for k in range(51):
        t[HIST + k * BINS + 18] += 4                         # [8, 12) mm
    k = 17 + 3
    t[HIST + k * BINS + 18] -= 1
    t[HIST + k * BINS + 15] += 1                             # one pose in [-4, 0) mm
    t[n_groups * ROW] = 3                                    # ignored
    return t
