"""Host restatement and seeded inputs of the regressor report (tests/test_regressor_report.py, tests/test_gpu_regressor_report.py).

Written from include/jrr.h: the table layout JRR_SHIFT_ACC_*, the arithmetic of jrr_regressor_shift_accumulate (every operation
rounded once, in the order written there -- numpy rounds every float32 operation once, and nothing here is fused) and the inside
rule of jrr_draw_discs.  `dtype` float32 follows the kernel; float64 is the yardstick the derived numbers are measured against.
Inputs are regenerated from numpy.random.RandomState seeds, never stored."""
import struct
import zlib

import numpy as np

F32, F64 = np.float32, np.float64
NJ = 17
ROW, TRAILER = 1277, 2
COUNT, BAD, SUM, MOM, ABS, ABS_REL, HIST, BINS = 0, 1, 2, 53, 155, 172, 189, 64
R_HIP, L_HIP, PELVIS, NECK = 1, 4, 0, 8
MOM_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))

# a canonical upright H36M skeleton in SMPL's axes (x to the body's left, y up, z forward), metres, pelvis at the origin
UPRIGHT = np.array([[0, 0, 0], [-0.13, 0, 0], [-0.13, -0.45, 0], [-0.13, -0.9, 0], [0.13, 0, 0], [0.13, -0.45, 0], [0.13, -0.9, 0],
                    [0, 0.25, 0], [0, 0.5, 0], [0, 0.6, 0.08], [0, 0.7, 0], [0.18, 0.45, 0], [0.45, 0.45, 0], [0.7, 0.45, 0],
                    [-0.18, 0.45, 0], [-0.45, 0.45, 0], [-0.7, 0.45, 0]], dtype=F64)


# ---- the restatement: body frame and displacements --------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def shift_terms(ja, jb, dtype=F32):
    """per pose what jrr_regressor_shift_accumulate forms before it rounds to integers, in `dtype`: dict with frame (B,3,3) rows
    xh, yh, zh; c (B,17,3) body-frame displacement; length (B,17); rel (B,17) pelvis-relative length; good (B,) bool"""
    a, b = np.asarray(ja, dtype=F32).astype(dtype), np.asarray(jb, dtype=F32).astype(dtype)
    with np.errstate(all='ignore'):
        finite = np.isfinite(a).reshape(a.shape[0], -1).all(1) & np.isfinite(b).reshape(b.shape[0], -1).all(1)
        x, u = a[:, L_HIP] - a[:, R_HIP], a[:, NECK] - a[:, PELVIS]
        lx = np.sqrt(_dot(x, x))
        xh = x / lx[:, None]
        z = _cross(xh, u)
        lu, lz = np.sqrt(_dot(u, u)), np.sqrt(_dot(z, z))
        zh = z / lz[:, None]
        yh = _cross(zh, xh)
        d = b - a
        c = np.stack([_dot(d, xh[:, None]), _dot(d, yh[:, None]), _dot(d, zh[:, None])], axis=-1)
        length = np.sqrt(_dot(d, d))
        r = d - d[:, :1]
        rel = np.sqrt(_dot(r, r))
        good = finite & (lx >= dtype(F32(1e-4))) & (lz >= dtype(F32(1e-4)) * lu) & (np.abs(c) < dtype(4.0)).reshape(a.shape[0], -1).all(1)
    return {'frame': np.stack([xh, yh, zh], axis=1), 'c': c, 'length': length, 'rel': rel, 'good': good}


def _fixed(x32):
    """llrintf(x * 2^24): the scaling is exact in float32, np.rint rounds ties to even"""
    return np.rint((x32 * F32(16777216.0)).astype(F32).astype(F64)).astype(np.int64)


def accumulate(ja, jb, group, n_groups: int, table=None) -> np.ndarray:
    """ADD to `table` (int64, n_groups * 1277 + 2; None = zeros) what jrr_regressor_shift_accumulate adds, in exact integers"""
    table = np.zeros(n_groups * ROW + TRAILER, dtype=np.int64) if table is None else table.copy()
    t = shift_terms(ja, jb, F32)
    B = t['good'].shape[0]
    group = np.zeros(B, dtype=np.int32) if group is None else np.asarray(group)
    for b, g in enumerate(group.tolist()):
        if g < 0:
            table[n_groups * ROW + 0] += 1
            continue
        if g >= n_groups:
            table[n_groups * ROW + 1] += 1
            continue
        row = table[g * ROW:(g + 1) * ROW]
        if not t['good'][b]:
            row[BAD] += 1
            continue
        row[COUNT] += 1
        q = _fixed(t['c'][b])                                                       # (17,3)
        row[SUM:SUM + NJ * 3] += q.reshape(-1)
        mom = np.stack([(q[:, i] * q[:, k]) >> 16 for i, k in MOM_PAIRS], axis=1)   # arithmetic shift of the int64 product
        row[MOM:MOM + NJ * 6] += mom.reshape(-1)
        row[ABS:ABS + NJ] += _fixed(t['length'][b])
        row[ABS_REL:ABS_REL + NJ] += _fixed(t['rel'][b])
        bins = np.clip(np.floor((t['length'][b] * F32(500.0)).astype(F32)).astype(np.int64), 0, BINS - 1)
        np.add.at(row, HIST + np.arange(NJ) * BINS + bins, 1)
    return table


def reference_stats(ja, jb, keep):
    """float64 yardstick of the derived numbers over the poses `keep` (bool (B,)) that are good: mean (17,3), std (17,3) (population),
    mean length (17), mean pelvis-relative length (17), all in metres, and the count"""
    t = shift_terms(ja, jb, F64)
    use = np.asarray(keep, dtype=bool) & t['good']
    if not use.any():
        return {'n': 0}
    c = t['c'][use]
    return {'n': int(use.sum()), 'mean': c.mean(0), 'std': c.std(0), 'mean_abs': t['length'][use].mean(0), 'mean_rel': t['rel'][use].mean(0)}


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------
def rotations(n: int, rs) -> np.ndarray:
    """(n,3,3) proper rotations, uniformly random"""
    q = rs.randn(n, 4)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], axis=1)


def bodies(B: int, seed: int):
    """(A (B,17,3) float64, R (B,3,3), t (B,3)): the upright skeleton with 3 cm of joint noise under random rigid motions"""
    rs = np.random.RandomState(seed)
    local = UPRIGHT[None] + rs.randn(B, NJ, 3) * 0.03
    R, t = rotations(B, rs), rs.randn(B, 3) * 0.3
    return np.einsum('brc,bjc->bjr', R, local) + t[:, None], R, t


def shift_case(B: int, seed: int = 51, n_groups: int = 3):
    """(joints_a, joints_b float32 (B,17,3), group int32 (B,)): B - A is a per-joint offset in the body's own axes (millimetres to
    centimetres, with a spread of a few millimetres) turned into the world; groups 0 .. 2.  From B >= 67: ids -1 (poses 5, 44) and 3
    (pose 9), a NaN pose (7), a pose with coincident hips (11) and one with a 5 m displacement of one joint along the body's x (13)."""
    A, R, _ = bodies(B, seed)
    rs = np.random.RandomState(seed + 1)
    offset = rs.randn(NJ, 3) * 0.012
    local = offset[None] + rs.randn(B, NJ, 3) * 0.004
    Bj = A + np.einsum('brc,bjc->bjr', R, local)
    ja, jb = A.astype(F32), Bj.astype(F32)
    group = (np.arange(B) % n_groups).astype(np.int32)
    if B >= 67:
        group[[5, 44]] = -1
        group[9] = n_groups
        jb[7, 3, 1] = np.nan
        ja[11, L_HIP] = ja[11, R_HIP]
        jb[13, 6] += (R[13] @ np.array([5.0, 0.0, 0.0])).astype(F32)     # along the body's own x: the component itself passes the cap
    return ja, jb, group


def moved(ja, jb, seed: int):
    """the same poses under one random rotation and translation per pose (computed in float64, rounded to float32 once)"""
    rs = np.random.RandomState(seed)
    B = ja.shape[0]
    R, t = rotations(B, rs), rs.randn(B, 3) * 0.3
    f = lambda j: (np.einsum('brc,bjc->bjr', R, j.astype(F64)) + t[:, None]).astype(F32)
    return f(ja), f(jb)


# ---- the restatement: discs --------------------------------------------------------------------------------------------------
def draw_discs(rgb, points, colours, radius=None, radii=None) -> np.ndarray:
    """what jrr_draw_discs leaves in a copy of rgb (B,h,w,3) uint8: points (n_sets,B,n_pts,2) float32, radii (n_sets,B,n_pts) or the
    scalar radius; pixel (x, y) is inside iff dx * dx + dy * dy <= r * r in float32, sets and points painted in order"""
    out = np.array(rgb, dtype=np.uint8, copy=True)
    B, h, w, _ = out.shape
    pts = np.asarray(points, dtype=F32)
    xs, ys = np.arange(w, dtype=F32), np.arange(h, dtype=F32)
    colours = np.asarray(colours, dtype=np.uint8).reshape(-1, 3)
    with np.errstate(all='ignore'):
        for s in range(pts.shape[0]):
            for b in range(B):
                for p in range(pts.shape[2]):
                    px, py = pts[s, b, p]
                    r = F32(radius) if radii is None else F32(radii[s, b, p])
                    if not (np.isfinite(px) and np.isfinite(py) and np.isfinite(r)) or r < 0:
                        continue
                    dx, dy = xs - px, ys - py
                    inside = ((dx * dx)[None, :] + (dy * dy)[:, None]) <= r * r
                    out[b][inside] = colours[s]
    return out


def disc_case(h: int, w: int, n_sets: int, seed: int, B: int = 2, n_random: int = 6):
    """(rgb (B,h,w,3) random bytes, points (n_sets,B,P,2), radii (n_sets,B,P), colours (n_sets,3)): per set and picture the edge cases
    -- off the picture, on its border, exact pixel centres with r = 0, r < 0, NaN / inf coordinates and radii, a large disc shared by
    all sets (the later set wins) -- then random discs"""
    rs = np.random.RandomState(seed)
    rgb = rs.randint(0, 256, size=(B, h, w, 3)).astype(np.uint8)
    cx, cy = F32((w - 1) // 2), F32((h - 1) // 2)
    fixed = [(-50.0, -50.0, 3.0), (w + 30.0, cy, 4.0),                               # off the picture
             (-2.0, cy, 3.5), (w - 1.0, h - 1.0, 1.0), (0.0, 0.0, 1.5), (w - 0.5, 0.25, 2.0),   # on / across the border
             (cx, cy, 0.0), (0.0, h - 1.0, 0.0), (cx + 0.5, cy, 0.0),                 # r = 0: exactly one pixel / none off-centre
             (cx, cy, -1.0), (np.nan, cy, 3.0), (cx, np.inf, 3.0), (cx, cy, np.nan), (cx, cy, np.inf), (cx, -np.inf, 2.0),
             (cx / 2, cy / 2, min(h, w) / 3.0)]                                       # shared by every set
    P = len(fixed) + n_random
    points = np.zeros((n_sets, B, P, 2), dtype=F32)
    radii = np.zeros((n_sets, B, P), dtype=F32)
    for s in range(n_sets):
        for b in range(B):
            order = rs.permutation(len(fixed))
            for k, i in enumerate(order):
                points[s, b, k] = fixed[i][:2]
                radii[s, b, k] = fixed[i][2]
            points[s, b, len(fixed):, 0] = rs.uniform(-3, w + 3, n_random)
            points[s, b, len(fixed):, 1] = rs.uniform(-3, h + 3, n_random)
            radii[s, b, len(fixed):] = rs.uniform(0, max(1.0, min(h, w) / 8.0), n_random)
    colours = rs.randint(0, 256, size=(n_sets, 3)).astype(np.uint8)
    return rgb, points, radii, colours


# ---- files -------------------------------------------------------------------------------------------------------------------
def read_png(path: str) -> np.ndarray:
    """an 8-bit RGB, non-interlaced PNG whose scanlines all use filter 0 (what report.write_png writes): (H,W,3) uint8"""
    data = open(path, 'rb').read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    at, idat, shape = 8, b'', None
    while at < len(data):
        n, tag = struct.unpack('>I', data[at:at + 4])[0], data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        if tag == b'IHDR':
            w, h, depth, colour, _, _, interlace = struct.unpack('>IIBBBBB', body)
            assert (depth, colour, interlace) == (8, 2, 0)
            shape = (h, w)
        elif tag == b'IDAT':
            idat += body
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(shape[0], 1 + 3 * shape[1])
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(shape[0], shape[1], 3).copy()
