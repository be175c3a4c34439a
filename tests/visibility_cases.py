"""Inputs and the host restatement of `--visible_refined` (include/jrr.h: jrr_point_visibility, jrr_visibility_accumulate; DESIGN.md
section 3v), shared by tests/test_visibility.py and tests/test_gpu_visibility.py.  Nothing is stored: every input is seeded.

The restatement is written from the header's definition alone: the Moeller-Trumbore form with origin 0 (e1 = b - a, e2 = c - a,
h = p x e2, det = e1 . h, u = -(a . h) / det, q = -(a x e1), v = (p . q) / det, s = (e2 . q) / det; lambda = (1 - u - v, u, v)), every
operation a numpy ufunc of its own, in float64 or in float32.  The pixel of bit 1 is restated in float32 operation for operation.

Sure queries.  Next to the decision itself (min lambda >= 0, s > 0, s d < d - margin) the float64 run takes it under two shifts:
strict (min lambda >= +TAU, z_hit <= d - margin - DZ) and loose (min lambda >= -TAU, z_hit <= d - margin + DZ), TAU = 1e-3 (about four
times the 2.7e-4 a float32 run of this form deviates from float64 on near-edge barycentrics of a body with 1 cm triangles at 4 m),
DZ = 0.1 mm.  strict <= exact <= loose face by face, so a query whose strict and loose COUNTS agree has that count under any rounding
inside the band, and one whose strict and loose BITS agree has that bit.  Only those are compared with float32 results; the caps
below bound how many a case may leave out, and tests/test_visibility.py asserts them on the float64 numbers alone.
"""
import functools
import importlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import depth_cases as dc
import penetration_cases as pc
from conftest import PKG_NAME

F32, F64 = np.float32, np.float64
TAU, DZ = 1e-3, 1e-4
CAP_BIT, CAP_COUNT, CAP_JOINTS = 0.01, 0.02, 2
OCCLUDED, OUTSIDE, INVALID = 1, 2, 4
NJ = 17
# the table row (include/jrr.h, JRR_VIS_ACC_*)
ROW, TRAILER, PARTS = 154, 2, 32
COUNT, BAD, SUM_VERT_SEEN, SUM_VERT_OCCLUDED, SUM_VERT_OUTSIDE = 0, 1, 2, 3, 4
J_SEEN, J_OCCLUDED, J_OUTSIDE, SUM_ERR_SEEN, SUM_ERR_OCCLUDED, PART_SEEN, PART_ALL = 5, 22, 39, 56, 73, 90, 122
ERR_CAP = F32(1.0e5)
PLACE_BAD_BITS = 7
MARGIN = 0.005


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


# ---- the restatement -------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _counts_chunk(a, e1, e2, q, e2q, face_ok, fidx, p, pidx, margin, dtype, shifts):
    """p (P,3) against all faces -> [count (P,) per (tau, dz) of `shifts`]"""
    P = p[:, None, :]
    h = _cross(P, e2[None])
    det = _dot(e1[None], h)
    with np.errstate(all='ignore'):
        u = -_dot(a[None], h) / det
        v = _dot(P, q[None]) / det
        s = e2q[None] / det
        lam = np.minimum(np.minimum((dtype(1) - u) - v, u), v)
        d = p[:, 2][:, None]
        z = s * d
        ok = face_ok[None] & (det != 0) & (s > 0)
        if pidx is not None:                                            # the query is a vertex: skip the faces that name it
            ok = ok & (fidx[None, :, 0] != pidx[:, None]) & (fidx[None, :, 1] != pidx[:, None]) & (fidx[None, :, 2] != pidx[:, None])
        out = []
        for tau, dz in shifts:
            hit = ok & (lam >= dtype(tau)) & ((z < (d - dtype(margin)) - dtype(dz)) if dz == 0 else (z <= (d - dtype(margin)) - dtype(dz)))
            out.append(hit.sum(1).astype(np.int32))
    return out


def counts(verts, faces, points, margin, dtype=F64, shifts=((0.0, 0.0),), chunk=128):
    """one pose: verts (V,3), faces (F,3), points (P,3) or None (the vertices, faces that name the query skipped) -> [count (P,) int32
    per shift]; a query with d <= 0 or a non-finite coordinate counts 0.  A face with an index out of range, a non-finite corner or a
    zero (b - a) x (c - a) adds nothing."""
    verts = np.asarray(verts, dtype=dtype)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    self_q = points is None
    p = verts if self_q else np.asarray(points, dtype=dtype)
    n = p.shape[0]
    if faces.shape[0] == 0:
        return [np.zeros(n, np.int32) for _ in shifts]
    inr = ((faces >= 0) & (faces < verts.shape[0])).all(1)
    f = np.where(inr[:, None], faces, 0)
    with np.errstate(all='ignore'):
        a, b, c = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
        e1, e2 = b - a, c - a
        nrm = _cross(e1, e2)
        q = -_cross(a, e1)
        e2q = _dot(e2, q)
        face_ok = inr & np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1) & (nrm != 0).any(1)
    valid = np.isfinite(p).all(1) & (p[:, 2] > 0)
    psafe = np.where(valid[:, None], p, dtype(1))
    spans = [(i, min(n, i + chunk)) for i in range(0, n, chunk)]

    def work(span):
        i, j = span
        return _counts_chunk(a, e1, e2, q, e2q, face_ok, faces, psafe[i:j], np.arange(i, j) if self_q else None, margin, dtype, shifts)

    if len(spans) > 4:
        with ThreadPoolExecutor(8) as ex:
            parts = list(ex.map(work, spans))
    else:
        parts = [work(s) for s in spans]
    out = [np.concatenate([pt[k] for pt in parts]) for k in range(len(shifts))]
    return [np.where(valid, o, 0).astype(np.int32) for o in out]


SHIFTS = ((0.0, 0.0), (TAU, DZ), (-TAU, -DZ))


def pixel_outside(points, K, rect):
    """bit 1 in float32, operation for operation: points (B,P,3), K (B,3,3), rect (B,4) -> bool (B,P) (garbage where bit 2 is set)"""
    p, K, r = np.asarray(points, F32), np.asarray(K, F32), np.asarray(rect, F32)
    with np.errstate(all='ignore'):
        u = (K[:, None, 0, 0] * p[..., 0]) / p[..., 2] + K[:, None, 0, 2]
        v = (K[:, None, 1, 1] * p[..., 1]) / p[..., 2] + K[:, None, 1, 2]
        inside = (r[:, None, 0] <= u) & (u < r[:, None, 2]) & (r[:, None, 1] <= v) & (v < r[:, None, 3])
    return ~inside


def visibility(verts, faces, points, K, rect, margin, min_crossings, dtype=F64):
    """the batch: verts (B,V,3) float32, points (B,P,3) float32 or None -> dict(count, code, sure_count, sure_bit), each (B,P).
    dtype float64: sure_* from the two shifts; float32: sure_* all True (nothing to say)."""
    verts = np.asarray(verts, F32)
    B = verts.shape[0]
    pts = verts if points is None else np.asarray(points, F32)
    cnt, lo, hi = [], [], []
    for b in range(B):
        r = counts(verts[b], faces, None if points is None else pts[b], margin, dtype, SHIFTS if dtype is F64 else SHIFTS[:1])
        cnt.append(r[0])
        lo.append(r[1] if dtype is F64 else r[0])
        hi.append(r[2] if dtype is F64 else r[0])
    cnt, lo, hi = np.stack(cnt), np.stack(lo), np.stack(hi)
    invalid = ~(np.isfinite(pts).all(-1) & (pts[..., 2] > 0))
    code = np.where(cnt >= min_crossings, OCCLUDED, 0)
    if K is not None:
        code = code | np.where(pixel_outside(pts, K, rect), OUTSIDE, 0)
    code = np.where(invalid, INVALID, code).astype(np.uint8)
    return {'count': cnt, 'code': code, 'sure_count': (lo == hi) | invalid, 'sure_bit': ((lo >= min_crossings) == (hi >= min_crossings)) | invalid}


# ---- jrr_visibility_accumulate ----------------------------------------------------------------------------------------------
def fixed24(v):
    return np.rint(np.asarray(v, F32).astype(F64) * 16777216.0).astype(np.int64)      # e * 2^24 is exact in float32 below the cap


def accumulate(vcode, jcode, err, part, pose_status, group, n_groups, table=None, per_vertex=None):
    """the table (n_groups * ROW + TRAILER int64) and per_vertex (n_verts int64) after ADDING the poses, pose by pose"""
    vcode, jcode = np.asarray(vcode, np.uint8), np.asarray(jcode, np.uint8)
    B, n = vcode.shape
    t = np.zeros(n_groups * ROW + TRAILER, np.int64) if table is None else table.copy()
    pv = np.zeros(n, np.int64) if per_vertex is None else per_vertex.copy()
    lab = np.zeros(n, np.int64) if part is None else np.asarray(part).astype(np.int64)
    lab = np.where((lab >= 0) & (lab < PARTS), lab, PARTS - 1)
    for b in range(B):
        g = 0 if group is None else int(group[b])
        if g < 0:
            t[n_groups * ROW] += 1
            continue
        if g >= n_groups:
            t[n_groups * ROW + 1] += 1
            continue
        row = t[g * ROW:(g + 1) * ROW]
        bad = bool((vcode[b] & 0xFC).any() or (jcode[b] & 0xFC).any())
        bad = bad or (pose_status is not None and (int(pose_status[b]) & PLACE_BAD_BITS) != 0)
        bad = bad or (err is not None and not bool((np.asarray(err[b], F32) < ERR_CAP).all()))
        if bad:
            row[BAD] += 1
            continue
        row[COUNT] += 1
        row[SUM_VERT_SEEN] += int((vcode[b] == 0).sum())
        row[SUM_VERT_OCCLUDED] += int((vcode[b] & 1).sum())
        row[SUM_VERT_OUTSIDE] += int(((vcode[b] >> 1) & 1).sum())
        for j in range(NJ):
            m = int(jcode[b, j])
            seen, occ = m == 0, (m & 3) == 1
            row[J_SEEN + j] += seen
            row[J_OCCLUDED + j] += occ
            row[J_OUTSIDE + j] += (m >> 1) & 1
            if err is not None and (seen or occ):
                row[(SUM_ERR_SEEN if seen else SUM_ERR_OCCLUDED) + j] += int(fixed24(err[b, j]))
        row[PART_ALL:PART_ALL + PARTS] += np.bincount(lab, minlength=PARTS)
        row[PART_SEEN:PART_SEEN + PARTS] += np.bincount(lab[vcode[b] == 0], minlength=PARTS)
        pv += vcode[b] == 0
    return t, pv


# ---- cases -----------------------------------------------------------------------------------------------------------------
def square(z, half=1.0, n=1):
    """a square |x|, |y| <= half at depth z as a grid of 2 n^2 triangles: (verts ((n+1)^2,3), faces)"""
    g = np.linspace(-half, half, n + 1)
    v = np.array([[x, y, z] for y in g for x in g], F64)
    f = []
    for j in range(n):
        for i in range(n):
            k = j * (n + 1) + i
            f += [(k, k + 1, k + n + 2), (k, k + n + 2, k + n + 1)]
    return v, np.array(f, np.int32)


def sphere_at(centre, radius, levels=2):
    v, f = dc.sphere(levels)
    return v * radius + np.asarray(centre, F64), np.asarray(f, np.int32)


def camera(B, fx=1145.0, fy=1144.0, cx=512.5, cy=515.5):
    K = np.zeros((B, 3, 3), F32)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = fx, fy, cx, cy, 1
    K[:, 0, 1], K[:, 1, 0] = 7.0, -3.0                                     # entries nobody may read
    return K


@functools.lru_cache(maxsize=None)
def soup(n_faces, n_points, B, seed=0):
    """B poses of a triangle soup at depth 2 .. 3 m (n_faces triangles of about 0.6 m on 3 n_faces vertices) and n_points queries at
    depth 2.5 .. 4 m behind it, some behind the camera or not finite; a window that cuts the queries:
    dict(verts (B,3F,3) f32, faces (F,3) i32, points (B,P,3) f32, K, rect)"""
    rs = np.random.RandomState(1000 * n_faces + 10 * n_points + B + seed)
    centre = rs.uniform([-0.6, -0.6, 2.0], [0.6, 0.6, 3.0], size=(B, n_faces, 1, 3))
    verts = (centre + rs.uniform(-0.3, 0.3, size=(B, n_faces, 3, 3))).reshape(B, n_faces * 3, 3).astype(F32)
    faces = np.arange(n_faces * 3, dtype=np.int32).reshape(n_faces, 3)
    pts = rs.uniform([-0.9, -0.9, 2.5], [0.9, 0.9, 4.0], size=(B, n_points, 3)).astype(F32)
    flat = pts.reshape(-1, 3)
    if flat.shape[0] >= 8:
        flat[3, 2] = -1.0                                                  # behind the camera
        flat[5, 2] = 0.0                                                   # in the camera's plane
        flat[6, 0] = np.nan
        flat[7, 1] = np.inf
    rect = np.tile(F32([300.0, 250.0, 800.0, 700.0]), (B, 1))
    return {'verts': verts, 'faces': faces, 'points': pts, 'K': camera(B), 'rect': rect}


SOUP_SHAPES = ((1, 1, 1), (3, 63, 3), (4, 64, 1), (5, 65, 65), (20, 1025, 3), (20, 64, 65), (1, 65, 3))      # (n_faces, n_points, B)


def _rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


BODY_YAWS = (0.0, 0.7, np.pi / 2)
BODY_DEPTH = 4.0


@functools.lru_cache(maxsize=None)
def body_case():
    """the synthetic body of penetration_cases.body_meshes() -- template, side bend, moved bend -- turned by BODY_YAWS about the vertical
    and placed 4 m in front of the camera: dict(verts (3,6890,3) f32, faces (13776,3) i32, joints (3,17,3) f32: the first 17 of the
    model's joints, K, rect: a frame that cuts the body, part (6890,) i32)"""
    V, model = pc.body_meshes()
    V = np.stack([V[k] @ _rot_y(y).T + [0.05 * k, 0.1, BODY_DEPTH] for k, y in enumerate(BODY_YAWS)])
    joints = np.einsum('jv,bvc->bjc', np.asarray(model['J_regressor'], F64)[:NJ], V)
    part = np.argmax(np.asarray(model['lbs_weights']), axis=1).astype(np.int32)
    rect = np.tile(F32([0.0, 0.0, 1000.0, 600.0]), (3, 1))
    return {'verts': V.astype(F32), 'faces': np.asarray(model['faces']).astype(np.int32), 'joints': joints.astype(F32), 'K': camera(3),
            'rect': rect, 'part': part}


@functools.lru_cache(maxsize=None)
def body_reference(dtype_name='f64'):
    """(vertex queries, joint queries) of body_case(), each the dict of visibility()"""
    c = body_case()
    dtype = F64 if dtype_name == 'f64' else F32
    return (visibility(c['verts'], c['faces'], None, c['K'], c['rect'], MARGIN, 1, dtype),
            visibility(c['verts'], c['faces'], c['joints'], c['K'], c['rect'], MARGIN, 2, dtype))


@functools.lru_cache(maxsize=None)
def soup_reference(shape, dtype_name='f64', self_q=False):
    c = soup(*shape)
    dtype = F64 if dtype_name == 'f64' else F32
    return visibility(c['verts'], c['faces'], None if self_q else c['points'], c['K'], c['rect'], MARGIN, 1, dtype)


def check_caps(ref, what, joints=False):
    """the share of queries a case leaves out, per pose, against the caps; prints it"""
    for b in range(ref['count'].shape[0]):
        nb, nc, n = int((~ref['sure_bit'][b]).sum()), int((~ref['sure_count'][b]).sum()), ref['count'].shape[1]
        print(f'{what} pose {b}: {n} queries, bit 0 left out {nb} ({100.0 * nb / n:.2f} %), count left out {nc} ({100.0 * nc / n:.2f} %)')
        if joints:
            assert nb <= CAP_JOINTS and nc <= CAP_JOINTS, (what, b, nb, nc)
        else:
            assert nb <= CAP_BIT * n and nc <= CAP_COUNT * n, (what, b, nb, nc)


def hand_made_codes(seed=3, B=23, n_verts=300):
    """codes, errors, parts, statuses and groups that reach every word and every refusal of the accumulator:
    dict(vcode (B,n) u8, jcode (B,17) u8, err (B,17) f32 mm, part (n,) i32 with -1 and 40, pose_status (B,) i32, group (B,) i32 with -1
    and n_groups, n_groups)"""
    rs = np.random.RandomState(seed)
    vcode = rs.choice(np.array([0, 0, 0, 1, 1, 2, 3], np.uint8), size=(B, n_verts))
    jcode = rs.choice(np.array([0, 0, 1, 1, 2, 3], np.uint8), size=(B, NJ))
    err = rs.uniform(5.0, 120.0, size=(B, NJ)).astype(F32)
    part = rs.randint(0, 24, size=n_verts).astype(np.int32)
    part[7], part[11], part[12] = -1, 40, 31
    pose_status = np.zeros(B, np.int32)
    group = (np.arange(B) % 2).astype(np.int32)
    vcode[2, 17] = 4                                 # bit 2 among the vertices
    jcode[4, 3] = 4                                  # ... among the joints
    vcode[15, 0] = 255                               # a row nobody filled
    err[6, 2] = np.nan
    err[8, 16] = np.inf
    err[16, 5] = 2.0e5                               # absurd
    pose_status[9], pose_status[10], pose_status[12], pose_status[13] = 1, 2, 4, 8      # bit 3 does not void a pose
    group[11], group[14], group[20] = -1, 2, -7
    return {'vcode': vcode, 'jcode': jcode, 'err': err, 'part': part, 'pose_status': pose_status, 'group': group, 'n_groups': 2}


def host_operators(monkeypatch, engine, dtype=F32):
    """engine.point_visibility / evaluate_joints / visibility_accumulate on CPU tensors by the restatement (the GPU tests hold the kernels
    to it).  Returns the list every point_visibility call appends its dict to (count, code, sure_count, sure_bit), in call order."""
    import torch
    T = torch.from_numpy
    calls = []

    def point_visibility(verts_cam, faces, points_cam, K, rect, margin_m, min_crossings, status, want_count=True, out=None):
        r = visibility(verts_cam.numpy(), faces.numpy(), None if points_cam is None else points_cam.numpy(), None if K is None else K.numpy(),
                       None if rect is None else rect.numpy(), margin_m, min_crossings, dtype)
        calls.append(r)
        count, code = out
        code.copy_(T(r['code']))
        if count is not None:
            count.copy_(T(r['count']))
        return out

    def evaluate_joints(pred, target_mm):
        p = pred.double() - pred.double()[:, :1]
        e = ((p - target_mm.double() / 1000).norm(dim=2)).float()
        return e, e

    def visibility_accumulate(vcode, jcode, err, part, pose_status, group, n_groups, acc, per_vertex=None):
        t, pv = accumulate(vcode.numpy(), jcode.numpy(), None if err is None else err.numpy(), None if part is None else part.numpy(),
                           None if pose_status is None else pose_status.numpy(), None if group is None else group.numpy(), n_groups)
        acc += T(t)
        if per_vertex is not None:
            per_vertex += T(pv)

    for f in (point_visibility, evaluate_joints, visibility_accumulate):
        monkeypatch.setattr(engine, f.__name__, f)
    return calls
