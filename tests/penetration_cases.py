"""Host restatement and seeded inputs of the self-penetration report (tests/test_penetration_report.py, tests/test_gpu_penetration.py).

Written from include/jrr.h: the solid angle of jrr_point_mesh_depth as jrr_mesh_winding sums it (face f to partial sum f mod 4, each in
ascending order, then (s0 + s1) + (s2 + s3), in float64; divided by 4 pi, rounded to float once), the classification and the table
layout JRR_PEN_ACC_* of jrr_penetration_accumulate.  `dtype` float32 follows the kernel (each Omega in float32), float64 is the
yardstick.  The kernel may fuse products into sums, numpy does not: `wind` is compared within `depth_cases.bound(d)`, d being the
float32 restatement's own distance from the float64 one on the same inputs; the integer k and the three flags are compared exactly at
every point whose float64 |w| lies within 0.1 of an integer (`sure`), and the points left out are at most 1 % of a case.  The
accumulator is integers and compared word for word.  Inputs are regenerated from seeds, never stored."""
import functools
import importlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import depth_cases as dc
import mesh_shade_cases as mc
from conftest import PKG_NAME

F32, F64 = np.float32, np.float64
ROW, TRAILER, BINS, PARTS = 55, 2, 16, 32
COUNT, BAD, POSES_PEN, POSES_PEN8, SUM_PEN, SUM_THIN, SUM_UNSURE, HIST, PART = 0, 1, 2, 3, 4, 5, 6, 7, 23
MAX_POINTS = 65536
UNSURE_CAP = 0.01


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


# ---- the restatement -------------------------------------------------------------------------------------------------------
def _omega_sum(v, f, ok, p, dtype):
    """(P,) float64: the four partial sums of the solid angles of the faces f (corners in v) seen from the points p, and their tree"""
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    P = p[:, None, :]
    with np.errstate(all='ignore'):
        A, B, C = a - P, b - P, c - P
        la, lb, lc = np.sqrt(dc._dot(A, A)), np.sqrt(dc._dot(B, B)), np.sqrt(dc._dot(C, C))
        num = dc._dot(A, dc._cross(B, C))
        dn = la * lb * lc + dc._dot(A, B) * lc + dc._dot(B, C) * la + dc._dot(C, A) * lb
        omega = np.where(ok[None, :], dtype(2) * np.arctan2(num, dn), 0).astype(dtype).astype(F64)      # a skipped face adds nothing
        s = []
        for u in range(4):
            part = omega[:, u::4]
            if part.shape[1] > 64:               # a long sum in double: numpy's order moves it by 1e-15, far below the float32 of Omega
                s.append(part.sum(axis=1))
                continue
            acc = np.zeros(p.shape[0])
            for k in range(part.shape[1]):       # ascending, one add at a time
                acc = acc + part[:, k]
            s.append(acc)
        return (s[0] + s[1]) + (s[2] + s[3])


def winding(verts, faces, points, dtype=F64, chunk=256):
    """one pose: verts (V,3), faces (F,3), points (P,3) -> (wind (P,) in `dtype`, status): NaN for every point of a pose with a
    non-finite vertex and for a point with a non-finite coordinate; a face with an index outside [0, V) is skipped, status bit 0"""
    v, p = np.asarray(verts).astype(dtype), np.asarray(points).astype(dtype)
    f = np.asarray(faces).astype(np.int64)
    ok = ((f >= 0) & (f < v.shape[0])).all(axis=1)
    fs = np.where(ok[:, None], f, 0)
    spans = [(s, min(s + chunk, p.shape[0])) for s in range(0, p.shape[0], chunk)]
    with ThreadPoolExecutor(max_workers=8) as ex:
        total = np.concatenate(list(ex.map(lambda ab: _omega_sum(v, fs, ok, p[ab[0]:ab[1]], dtype), spans)))
    poisoned = ~np.isfinite(np.asarray(points, dtype=F64)).all(axis=1) | (not np.isfinite(np.asarray(verts, dtype=F64)).all())
    with np.errstate(all='ignore'):
        return np.where(poisoned, np.nan, total / (4.0 * np.pi)).astype(dtype), int((~ok).any())


def winding_batch(verts, faces, points, dtype=F64):
    """verts (B,V,3), points (B,P,3) -> (wind (B,P), status)"""
    rows = [winding(verts[b], faces, points[b], dtype) for b in range(verts.shape[0])]
    return np.stack([r[0] for r in rows]), int(any(r[1] for r in rows))


def classify(wind):
    """(k, penetrating, thin, unsure) of winding numbers, every operation in float32 rounded once, as the header writes them"""
    w = np.asarray(wind, dtype=F32)
    with np.errstate(invalid='ignore'):
        aw = np.abs(w)
        k = np.rint(aw)
        return k, k >= F32(2), k == F32(0), np.abs((aw - k).astype(F32)) > F32(0.1)


def sure(wind64):
    """the points whose integer is no matter of rounding: float64 |w| within 0.1 of an integer"""
    aw = np.abs(np.asarray(wind64, dtype=F64))
    with np.errstate(invalid='ignore'):
        return np.abs(aw - np.rint(aw)) <= 0.1


def n_bits(n):
    return int(n).bit_length()


# ---- the accumulator -------------------------------------------------------------------------------------------------------
def accumulate(wind, part, group, n_groups, table=None, per_vertex=None):
    """ADD to `table` (int64, n_groups * 55 + 2; None = zeros) and `per_vertex` (int64 (n_verts,)) what jrr_penetration_accumulate adds,
    in exact integers -> (table, per_vertex, counts (3,B) int32: n_pen, n_thin, n_unsure of every pose, whatever its group)"""
    wind = np.asarray(wind, dtype=F32)
    B, V = wind.shape
    t = np.zeros(n_groups * ROW + TRAILER, dtype=np.int64) if table is None else table
    pv = np.zeros(V, dtype=np.int64) if per_vertex is None else per_vertex
    counts = np.zeros((3, B), dtype=np.int32)
    for b in range(B):
        k, pen, thin, uns = classify(wind[b])
        counts[:, b] = pen.sum(), thin.sum(), uns.sum()
        g = 0 if group is None else int(group[b])
        if g < 0:
            t[n_groups * ROW] += 1
            continue
        if g >= n_groups:
            t[n_groups * ROW + 1] += 1
            continue
        row = t[g * ROW:(g + 1) * ROW]
        if not np.isfinite(wind[b]).all():
            row[BAD] += 1
            continue
        n_pen = int(pen.sum())
        row[COUNT] += 1
        row[POSES_PEN] += n_pen >= 1
        row[POSES_PEN8] += n_pen >= 8
        row[SUM_PEN] += n_pen
        row[SUM_THIN] += int(thin.sum())
        row[SUM_UNSURE] += int(uns.sum())
        row[HIST + min(BINS - 1, n_bits(n_pen))] += 1
        for v in np.flatnonzero(pen):
            l = 0 if part is None else int(part[v])
            row[PART + (l if 0 <= l < PARTS else PARTS - 1)] += 1
            pv[v] += 1
    return t, pv, counts


# ---- meshes ------------------------------------------------------------------------------------------------------------------
def merge(meshes):
    """[(verts, faces)] -> one vertex list, one face list and the component of every vertex"""
    V, Fc, L, base = [], [], [], 0
    for k, (v, f) in enumerate(meshes):
        V.append(np.asarray(v, dtype=F64))
        Fc.append(np.asarray(f) + base)
        L.append(np.full(len(v), k, dtype=np.int32))
        base += len(v)
    return np.concatenate(V), np.concatenate(Fc).astype(np.int32), np.concatenate(L)


def _spheres(levels, centres, radii, push=0.02):
    """spheres as one mesh; the points are its vertices pushed `push` towards their own sphere's centre"""
    v, f = dc.sphere(levels)
    verts, faces, label = merge([(v * r + np.asarray(c, dtype=F64), f) for c, r in zip(centres, radii)])
    pts = np.concatenate([v * (r - push) + np.asarray(c, dtype=F64) for c, r in zip(centres, radii)])
    return verts, faces, label, pts


def _make(name):
    if name == 'two_spheres':
        return _spheres(2, [(0, 0, 0), (1.0, 0, 0)], [1.0, 1.0])
    if name == 'nested':
        return _spheres(2, [(0, 0, 0), (0.1, 0.05, 0)], [1.0, 0.3])
    if name == 'three_spheres':
        h = 0.6 * np.sqrt(3) / 2
        return _spheres(2, [(0, 0, 0), (0.6, 0, 0), (0.3, h, 0)], [1.0, 1.0, 1.0])
    if name == 'row':
        return _spheres(3, [(1.2 * k, 0.05 * k, 0) for k in range(5)], [1.0] * 5)
    if name == 'octa_cube':
        verts, faces, label = merge([dc.octahedron(), dc.cube()])
        rs = np.random.RandomState(51)
        return verts, dc._relabel(faces), label, rs.uniform(-1.1, 1.1, size=(200, 3))
    raise KeyError(name)


SMALL = ('two_spheres', 'nested', 'three_spheres', 'octa_cube', 'row')


@functools.lru_cache(maxsize=None)
def small_case(name):
    """dict(verts (1,V,3) f32, faces (F,3) i32, points (1,P,3) f32, part (V,) i32: the component of every vertex)"""
    verts, faces, label, pts = _make(name)
    return {'verts': verts[None].astype(F32), 'faces': faces, 'points': pts[None].astype(F32), 'part': label}


BEND_JOINTS, BEND_ANGLE, PUSH_MM = (3, 6, 9), 1.0, 2.0


def _rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])


def body_meshes():
    """(3,6890,3) float64: the synthetic body's template, the side bend (SMPL joints 3, 6, 9 each rotated 1 rad about z, betas 0;
    float64 LBS), and the bend after a rigid motion"""
    sm = _mod('smpl_model')
    model = sm.synthetic_smpl()
    R = np.tile(np.eye(3), (2, 24, 1, 1))
    for j in BEND_JOINTS:
        R[1, j] = _rot_z(BEND_ANGLE)
    v = sm._lbs_np(model, R, np.zeros((2, 10)))
    rs = np.random.RandomState(61)
    Q, t = dc._rotation(rs), rs.uniform(-0.3, 0.3, size=3)
    return np.stack([v[0], v[1], v[1] @ Q.T + t]), model


def pushed(verts32, faces, offset_mm, sign):
    """the points of the report: x + t n in float32, t = -sign * offset, n the float32 vertex normals of jrr_vertex_normals"""
    n = mc.vertex_normals_ref(verts32, faces, F32)
    t = F32(-sign * (offset_mm / 1000.0))
    return (verts32 + (t * n).astype(F32)).astype(F32)


def orientation(verts, faces):
    v, f = np.asarray(verts, dtype=F64), np.asarray(faces).astype(np.int64)
    vol = np.einsum('fc,fc->', v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]]))
    assert vol != 0
    return 1 if vol > 0 else -1


@functools.lru_cache(maxsize=None)
def body_case():
    """dict(verts (3,6890,3) f32, faces (13776,3) i32, points (3,6890,3) f32: every vertex pushed 2 mm under the skin, part (6890,) i32:
    the joint with the largest skinning weight, sign: the orientation of the faces, model)"""
    V, model = body_meshes()
    V = V.astype(F32)
    faces = np.asarray(model['faces']).astype(np.int32)
    sign = orientation(V[0], faces)
    part = np.argmax(np.asarray(model['lbs_weights']), axis=1).astype(np.int32)
    return {'verts': V, 'faces': faces, 'points': pushed(V, faces, PUSH_MM, sign), 'part': part, 'sign': sign, 'model': model}


def case(name):
    return body_case() if name == 'body' else small_case(name)


@functools.lru_cache(maxsize=None)
def reference(name, dtype_name='f64'):
    """the winding numbers of the whole case, (B,P) in the named format, computed once and shared; callers slice and do not write"""
    c = case(name)
    w, status = winding_batch(c['verts'], c['faces'], c['points'], F64 if dtype_name == 'f64' else F32)
    assert status == 0
    w.setflags(write=False)
    return w


def distance(name):
    """d: the float32 restatement's distance from the float64 one, over the points that are finite in both"""
    return float(np.nanmax(np.abs(reference(name, 'f32').astype(F64) - reference(name))))


def check_cap(name):
    """at most 1 % of the case's points are left out of the exact comparisons; -> the mask of the points compared"""
    ok = sure(reference(name))
    assert (~ok).mean() <= UNSURE_CAP, (name, int((~ok).sum()), ok.size)
    return ok


# ---- the driver ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def driver_case():
    """6 meshes in two groups: template, bend, rigid copy of the bend, then a rigid copy of each of the three -> dict(verts (6,6890,3)
    f32, ids, names, faces, part, sign, source: the row of body_case() each mesh is a (moved) copy of)"""
    c = body_case()
    V64, _ = body_meshes()
    rs = np.random.RandomState(62)
    more = []
    for k in range(3):
        Q, t = dc._rotation(rs), rs.uniform(-0.3, 0.3, size=3)
        more.append(V64[k] @ Q.T + t)
    V = np.concatenate([c['verts'], np.stack(more).astype(F32)])
    return {'verts': V, 'ids': np.array([0, 1, 0, 1, 1, 0], dtype=np.int32), 'names': ['Walking', 'Sitting'], 'faces': c['faces'],
            'part': c['part'], 'sign': c['sign'], 'source': [0, 1, 2, 0, 1, 2]}


def hand_made_table(n_groups=2):
    """a table whose derived numbers are known: group 0 has 4 poses -- n_pen 0, 1, 9, 300 -- and one bad one, group 1 none; 3 ignored"""
    t = np.zeros(n_groups * ROW + TRAILER, dtype=np.int64)
    t[COUNT], t[BAD], t[POSES_PEN], t[POSES_PEN8] = 4, 1, 3, 2
    t[SUM_PEN], t[SUM_THIN], t[SUM_UNSURE] = 310, 4 * 689, 2
    for n in (0, 1, 9, 300):
        t[HIST + min(BINS - 1, n_bits(n))] += 1
    t[PART + 0], t[PART + 3], t[PART + 31] = 200, 100, 10
    t[n_groups * ROW] = 3
    pv = np.zeros(6890, dtype=np.int64)
    pv[:10], pv[100] = 3, 4
    return t, pv
