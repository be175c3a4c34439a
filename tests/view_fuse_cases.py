"""Host restatement and cases of the view fusion over the refined-pose table (jrr_view_relrot_accumulate, jrr_view_fuse;
refined.view_groups, refined.relative_rotations, refined.fuse_views).

Written from the definitions include/jrr.h states for the two entry points, in numpy for a chosen dtype; rot6d, unit_quat and conj_mul are
those of tests/refined_smooth_cases.py.  There is no reference implementation: the yardstick is float64.  The distance of the float32
evaluation of these functions from their float64 evaluation, on a test's own inputs, is what the GPU is held to:
`bound(d) = 3 d + 1e-7`.  Rotations are compared as matrices, angles in radians; a NaN must sit where the float64 evaluation has one.

float32 and float64 must take the same branch for that to mean anything.  `branch_margins` measures, in float64, per (group, joint):
the smallest |q_k . q_m| over two candidates (a sign), the smallest distance of a |q_k . q_a| from cos_half_max (the threshold) and the
gap between the least and the second-least cost (the anchor); `assert_branches` holds them to 1e-3, 1e-4 and 1e-4.  Two candidates tie
exactly by construction (q_0 . q_1 and q_1 . q_0 are the same products in the same order) and so do candidates that are the same bits
(the exact identity); both go to the first and are exempt from the cost gap.  The cases that are compared within `bound` are built so
that the conditions hold: one view of every group carries little noise (the medoid by a wide margin), the others 6 - 12 degrees.
The planted-truth case has independent noise on every view, as real fits have: its fused outputs are judged by their error against
the planted truth, never within `bound`, and of the three conditions it is held to the signs and the threshold (outside the replaced
views, which cannot meet them).
"""
import numpy as np

import refined_smooth_cases as sc
from refined_smooth_cases import bound, conj_mul, dist, dist_deg, dist_rot, rot6d, unit_quat  # noqa: F401

MAX_VIEWS, HALO, ACC_ROW, FIX = 8, 7, 12, 2.0 ** 24
N_ROWS, ROW = 96, 240
GROUP_SIZES = (1, 2, 3, 4, 8, 4, 4, 8, 4, 4, 4, 4, 4, 4, 8, 4)       # 70 positions; 26 .. 33 and 58 .. 65 straddle the tiles of 32
M = sum(GROUP_SIZES)
N_CAMS = 9                                                         # camera 8 is seen once, in a frame the reference camera misses
STATUS_INDEX, STATUS_MARKER, STATUS_WIDE, STATUS_PAIR = 1, 2, 4, 8


def cos_half(max_deg):
    """what the host passes: cos(max_deg / 2) rounded once from float64; 0 selects the plain mean"""
    return float(np.float32(np.cos(np.radians(float(max_deg)) / 2.0))) if max_deg > 0 else 0.0


# ---- the restatement ------------------------------------------------------------------------------------------------------
def qdot(a, b):
    p = a * b
    return p[..., 0] + p[..., 1] + p[..., 2] + p[..., 3]


def qmul(a, b):
    """a (x) b, every sum left to right"""
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def qconj(a):
    return a * np.array([1, -1, -1, -1], dtype=a.dtype)


def quats(x6d, dtype=np.float64):
    return unit_quat(rot6d(x6d, dtype), dtype)


def view_groups(scenes, cams, frames, has):
    """the lists refined.view_groups returns, from per-row scene / camera / frame (a negative frame: no key), by dictionaries"""
    rows = [i for i in range(len(has)) if has[i]]
    frames_of, seen, dups = {}, set(), {}
    for i in rows:
        if frames[i] < 0:
            continue
        key = (scenes[i], frames[i])
        if (key, cams[i]) in seen:
            dups.setdefault(key, []).append(i)
        else:
            seen.add((key, cams[i]))
            frames_of.setdefault(key, []).append(i)
    names = sorted({(scenes[i], cams[i]) for i in rows if frames[i] >= 0})
    order, group, pair, g = [], [], [], 0
    for key in sorted(frames_of):
        members = sorted(frames_of[key], key=lambda i: (cams[i], i))
        if len(members) > MAX_VIEWS:
            raise ValueError('too many views')
        order += members
        group += [g] * len(members)
        pair += [names.index((scenes[i], cams[i])) for i in members]
        g += 1
        for i in sorted(dups.get(key, []), key=lambda i: (cams[i], i)):
            order.append(i), group.append(g), pair.append(-1)
            g += 1
    for i in rows:
        if frames[i] < 0:
            order.append(i), group.append(g), pair.append(-1)
            g += 1
    ref_pair = [min(c for c, n in enumerate(names) if n[0] == scene) for scene, _ in names]
    as32 = lambda a: np.array(a, dtype=np.int32).reshape(-1)
    return as32(order), as32(group), as32(pair), as32(ref_pair), names, sum(len(v) for v in dups.values())


def valid_positions(table, order, group, pair, n_pairs):
    """(valid (M,) bool, status bits): a position that raises a bit is nobody's member"""
    Mn = len(order)
    valid, status = np.ones(Mn, bool), 0
    for p in range(Mn):
        bits = 0
        if not 0 <= order[p] < table.shape[0]:
            bits |= STATUS_INDEX
        elif not table[order[p], 229] == 1.0:
            bits |= STATUS_MARKER
        if pair[p] >= n_pairs:
            bits |= STATUS_PAIR
        if (p >= MAX_VIEWS and group[p - MAX_VIEWS] == group[p]) or (p + MAX_VIEWS < Mn and group[p + MAX_VIEWS] == group[p]):
            bits |= STATUS_WIDE
        valid[p] = bits == 0
        status |= bits
    return valid, status


def members_of(p, group, valid):
    return [n for n in range(max(0, p - HALO), min(len(group), p + HALO + 1)) if valid[n] and group[n] == group[p]]


def accumulate_table(x6d, group, pair, ref_pair, valid=None, positions=None):
    """the (n_pairs, 12) int64 table of the kernel, from the float32 evaluation: per counted position 1 and rint(float32(e_i e_j) 2^24) for
    the ten products ww wx wy wz xx xy xz yy yz zz of e = q_ref(joint 0) (x) conj(q_p(joint 0))"""
    Mn, n_pairs = len(group), len(ref_pair)
    valid = np.ones(Mn, bool) if valid is None else valid
    q0 = quats(x6d[:, 0], np.float32)
    acc = np.zeros((n_pairs, ACC_ROW), np.int64)
    iu = np.triu_indices(4)
    for p, ref in _counted(group, pair, ref_pair, valid, positions):
        e = qmul(q0[ref], qconj(q0[p]))
        prod = e[:, None] * e[None, :]
        assert prod.dtype == np.float32
        acc[pair[p], 0] += 1
        acc[pair[p], 1:11] += np.rint(prod[iu].astype(np.float64) * FIX).astype(np.int64)
    return acc


def _counted(group, pair, ref_pair, valid, positions=None):
    """(p, its group's reference-camera member) of the positions the accumulation counts"""
    for p in (range(len(group)) if positions is None else positions):
        c = pair[p]
        if not valid[p] or c < 0 or ref_pair[c] == c:
            continue
        ref = [n for n in members_of(p, group, valid) if n != p and pair[n] == ref_pair[c]]
        if ref:
            yield p, ref[0]


def accumulate(x6d, group, pair, ref_pair, dtype=np.float64, valid=None):
    """(count (n_pairs,) int64, mean (n_pairs, 4, 4) float64): per pair the mean of e e^T over the positions whose group holds the pair's
    reference camera.  float64: the mean of the float64 products.  float32: what the kernel stores (accumulate_table) over 2^24 count."""
    if dtype == np.float32:
        return acc_mean(accumulate_table(x6d, group, pair, ref_pair, valid))
    Mn, n_pairs = len(group), len(ref_pair)
    valid = np.ones(Mn, bool) if valid is None else valid
    q0 = quats(x6d[:, 0], np.float64)
    count, total = np.zeros(n_pairs, np.int64), np.zeros((n_pairs, 4, 4))
    for p, ref in _counted(group, pair, ref_pair, valid):
        e = qmul(q0[ref], qconj(q0[p]))
        count[pair[p]] += 1
        total[pair[p]] += e[:, None] * e[None, :]
    return count, total / np.maximum(count, 1)[:, None, None]


def acc_mean(acc):
    """the (n_pairs, 12) int64 table of the kernel as (count, mean (n_pairs, 4, 4) float64)"""
    acc = np.asarray(acc, dtype=np.int64)
    mean = np.zeros((acc.shape[0], 4, 4))
    iu = np.triu_indices(4)
    for c in range(acc.shape[0]):
        A = np.zeros((4, 4))
        A[iu] = acc[c, 1:11] / (FIX * max(1, int(acc[c, 0])))
        mean[c] = A + np.triu(A, 1).T
    return acc[:, 0].copy(), mean


def solve(count, mean, ref_pair):
    """(rel (n_pairs, 4) float32, residual_deg): the eigenvector of the largest eigenvalue with w >= 0; (1,0,0,0) for a reference camera,
    zeros for a pair nobody counted"""
    rel, res = np.zeros((len(count), 4)), np.full(len(count), np.nan)
    for c in range(len(count)):
        if ref_pair[c] == c:
            rel[c], res[c] = (1, 0, 0, 0), 0.0
        elif count[c] > 0:
            lam, U = np.linalg.eigh(mean[c])
            rel[c] = U[:, -1] * (1.0 if U[0, -1] >= 0 else -1.0)
            res[c] = np.degrees(2 * np.arccos(np.sqrt(min(1.0, max(0.0, lam[-1])))))
    return rel.astype(np.float32), res


def _fuse_block(Q, chm, dtype, margins=None):
    """Q (V, J, 4), the candidates of J joints in position order -> (f (J, 4), taken (V, J) bool)"""
    V, J = Q.shape[:2]
    one = dtype(1)
    dots = {(k, m): qdot(Q[k], Q[m]) for k in range(V) for m in range(V) if k != m}
    a = np.zeros(J, dtype=np.int64)
    if chm > 0:
        cost = np.zeros((V, J), dtype)
        for k in range(V):
            for m in range(V):
                if m != k:
                    cost[k] = cost[k] + (one - np.abs(dots[(k, m)]))
        a = np.argmin(cost, 0)                                      # the first of equal costs
    qa = Q[a, np.arange(J)]
    d = qdot(Q, qa[None])
    taken = (np.abs(d) >= dtype(chm)) if chm > 0 else np.ones((V, J), bool)
    s, started = np.zeros((J, 4), dtype), np.zeros(J, bool)
    for k in range(V):
        term = np.where((d[k] < 0)[:, None], -Q[k], Q[k])
        s = np.where((taken[k] & ~started)[:, None], term, np.where(taken[k][:, None], s + term, s))
        started |= taken[k]
    with np.errstate(all='ignore'):
        f = s / np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2] + s[:, 3] * s[:, 3])[:, None]
    assert f.dtype == dtype
    if margins is not None:
        inf = np.full(J, np.inf)
        sign = np.min([np.abs(v) for v in dots.values()], 0) if V > 1 else inf
        thr = np.abs(np.abs(d) - chm).min(0) if chm > 0 else inf
        gap = inf
        if chm > 0 and V > 2:
            srt = np.sort(cost, 0)
            gap = np.where((Q == Q[:1]).all((0, 2)), np.inf, srt[1] - srt[0])
        margins.append((sign, thr, gap))
    return f, taken


def fuse(x6d, betas, group, pair, rel, chm, dtype=np.float64, valid=None, margins=None):
    """the fusion over positions: x6d (M,24,6), betas (M,10), rel (n_pairs,4) float32, chm = cos_half(max_deg) -> a dict of x6d (M,24,6),
    betas (M,10), body, orient (M,) in `dtype`, members, dropped (M,) int32 and taken (M,24), the number of views taken per joint (0 where
    the position is no candidate).  `margins`: a list that receives (group's first position, joints, sign, threshold, gap) per block."""
    Mn, J = x6d.shape[0], x6d.shape[1]
    valid = np.ones(Mn, bool) if valid is None else np.asarray(valid, bool)
    rel = np.asarray(rel, dtype=np.float32).astype(dtype)
    q = quats(x6d, dtype)
    xin = np.asarray(x6d).astype(dtype)
    out = {'x6d': np.full((Mn, J, 6), np.nan, dtype), 'betas': np.full((Mn, betas.shape[1]), np.nan, dtype), 'body': np.full(Mn, np.nan, dtype),
           'orient': np.full(Mn, np.nan, dtype), 'members': np.zeros(Mn, np.int32), 'dropped': np.zeros(Mn, np.int32),
           'taken': np.zeros((Mn, J), np.int32)}
    cache = {}
    for p in range(Mn):
        if not valid[p]:
            continue
        mem = members_of(p, group, valid)
        key = tuple(mem)
        if key not in cache:
            got = []
            body = _fuse_block(q[mem, 1:], chm, dtype, got if margins is not None else None)
            cand0 = [n for n in mem if pair[n] >= 0 and rel[pair[n]].any()]
            q0 = qmul(rel[[pair[n] for n in cand0]], q[cand0, 0])[:, None] if cand0 else None
            orient = _fuse_block(q0, chm, dtype, got if margins is not None else None) if cand0 else None
            if margins is not None:
                margins.append((mem[0], np.arange(1, J)) + got[0])
                if cand0:
                    margins.append((mem[0], np.arange(1)) + got[1])
            b = np.asarray(betas)[mem[0]].astype(dtype)
            for n in mem[1:]:
                b = b + np.asarray(betas)[n].astype(dtype)
            cache[key] = (body, cand0, q0, orient, b / dtype(len(mem)))
        (f, taken), cand0, q0, orient, b = cache[key]
        me = mem.index(p)
        own = taken[me] & (taken.sum(0) == 1)
        out['x6d'][p, 1:] = np.where(own[:, None], xin[p, 1:], sc.quat_to_6d(f))
        ang = sc.angle_deg(conj_mul(q[p, 1:], f))
        out['body'][p] = _sum_in_order(ang) / dtype(J - 1)
        out['dropped'][p] = int((~taken[me]).sum())
        out['taken'][p, 1:] = taken.sum(0)
        out['x6d'][p, 0] = xin[p, 0]
        if p in (cand0 or []):
            me0 = cand0.index(p)
            f0, taken0 = orient
            if not (taken0[me0, 0] and taken0[:, 0].sum() == 1):
                out['x6d'][p, 0] = sc.quat_to_6d(conj_mul(rel[pair[p]], f0[0]))
            out['orient'][p] = sc.angle_deg(conj_mul(q0[me0, 0], f0[0]))
            out['dropped'][p] += int(not taken0[me0, 0])
            out['taken'][p, 0] = taken0[:, 0].sum()
        out['betas'][p] = b
        out['members'][p] = len(mem)
    for k in ('x6d', 'betas', 'body', 'orient'):
        assert out[k].dtype == dtype
    return out


def _sum_in_order(a):
    s = a[0]
    for j in range(1, a.shape[0]):
        s = s + a[j]
    return s


def assert_branches(margins, exempt=None, cost=True):
    """the conditions of the module docstring over what `fuse(..., margins=...)` collected; `exempt(first position, joint)` -> bool"""
    worst = [np.inf, np.inf, np.inf]
    for first, joints, sign, thr, gap in margins:
        for k, j in enumerate(joints):
            if exempt is not None and exempt(first, int(j)):
                continue
            worst = [min(worst[0], sign[k]), min(worst[1], thr[k]), min(worst[2], gap[k])]
    assert worst[0] > 1e-3, f'two candidates with |q . q| = {worst[0]:.3e}: their relative sign is not decided'
    assert worst[1] > 1e-4, f'a candidate {worst[1]:.3e} from the threshold'
    assert not cost or worst[2] > 1e-4, f'the two least costs differ by {worst[2]:.3e}'
    return worst


def distances(got, want):
    """(rotation, betas, body rad, orient rad) of two results of `fuse` (or of the kernel's outputs in that form)"""
    return (dist_rot(got['x6d'], want['x6d']), dist(got['betas'], want['betas']), dist_deg(got['body'], want['body']),
            dist_deg(got['orient'], want['orient']))


def rot_angle_deg(Ra, Rb):
    """the angle between rotation matrices (..., 3, 3), in degrees, float64"""
    tr = np.einsum('...ij,...ij->...', np.asarray(Ra, np.float64), np.asarray(Rb, np.float64))
    return np.degrees(np.arccos(np.clip((tr - 1) / 2, -1, 1)))


# ---- cases ----------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _noise(rng, n, lo_deg, hi_deg):
    """n rotations by lo .. hi degrees about random axes"""
    return sc.expmap(_unit(rng, n) * np.radians(rng.uniform(lo_deg, hi_deg, size=(n, 1))))


def group_views(rng, cams, E, rel, J=24, outlier=None):
    """(V, J, 6) float64: the views `cams` of one instant.  Per joint j a world rotation; joint 0 is seen as E[cam] W, the others as W,
    each times a view's noise: one view of the group (any) 0 - 1 degree, the others 6 - 12 degrees.  j % 4 selects 0: any angle, 1: within
    1e-3 of pi about axes some 3 degrees apart (the rotation moves by twice the axis), 2: the exact identity, 3: a quarter turn about an
    axis near -x, where Shepperd's branch -- and with it the quaternion's sign -- changes from view to view.  Except for the identity the
    two columns are scaled by 0.5 - 2 and perturbed: not orthonormal, as refined poses are.  `outlier` (view, joint): that view -- the
    next one, should it be the quiet view -- is turned by 60 degrees there.  A joint's views are drawn again until, in float64 and at 30
    degrees, no sign is closer to 0 than 1e-2, no candidate closer to the threshold than 1e-3 and the two least costs differ by 1e-3
    (joint 0: of the candidates under `rel` (9,4), the d the tests pass to the kernel)."""
    V = len(cams)
    quiet = rng.randint(V)
    if outlier is not None and outlier[0] == quiet:
        outlier = ((quiet + 1) % V, outlier[1])
    x = np.zeros((V, J, 6))
    for j in range(J):
        kind = j % 4
        lo, hi = np.where(np.arange(V) == quiet, 0.0, 6.0)[:, None], np.where(np.arange(V) == quiet, 1.0, 12.0)[:, None]
        for attempt in range(1000):
            noise = sc.expmap(_unit(rng, V) * np.radians(rng.uniform(lo, hi)))
            if kind == 0:
                W = sc.expmap(_unit(rng, 1) * rng.uniform(0, np.pi))[0]
                R = W[None] @ noise
            elif kind == 1:
                ax = _unit(rng, 1) + np.where(np.arange(V) == quiet, 0.002, 0.06)[:, None] * _unit(rng, V)
                ax /= np.linalg.norm(ax, axis=1, keepdims=True)
                R = sc.expmap(ax * (np.pi - rng.uniform(0, 1e-3, size=(V, 1))))
            elif kind == 2:
                x[:, j] = sc.to_6d(np.eye(3))
                break
            else:
                ax = np.array([-1.0, 0.0, 0.0]) + 0.1 * rng.normal(size=3)
                W = sc.expmap((ax / np.linalg.norm(ax))[None] * (np.pi / 2))[0]
                R = W[None] @ noise
            if outlier is not None and outlier[1] == j:
                R[outlier[0]] = R[outlier[0]] @ sc.expmap(_unit(rng, 1) * np.radians(60.0))[0]
            if j == 0:
                R = E[list(cams)] @ R
            x[:, j] = sc.to_6d(R) * np.repeat(rng.uniform(0.5, 2.0, size=(V, 1, 2)), 3, 1).reshape(V, 6) + rng.normal(scale=0.01, size=(V, 6))
            q = quats(x[:, j].astype(np.float32))
            if j == 0:
                known = rel[list(cams)].any(1)
                q = qmul(rel[list(cams)].astype(np.float64)[known], q[known])
            got = []
            if q.shape[0] > 1:
                _fuse_block(q[:, None], cos_half(30.0), np.float64, got)
            if not got or (got[0][0][0] > 1e-2 and got[0][1][0] > 1e-3 and got[0][2][0] > 1e-3):
                break
        else:
            raise AssertionError('no draw met the branch conditions')
    return x


def planted_rel(E, known):
    """(n, 4) float32: the quaternions of E_0 E_c^T with w >= 0, (1,0,0,0) for camera 0 and zeros where `known` is False"""
    q = quats(sc.to_6d(E[0][None] @ E.transpose(0, 2, 1)))
    q = np.where(q[:, :1] < 0, -q, q)
    q[0] = (1, 0, 0, 0)
    return np.where(np.asarray(known, bool)[:, None], q, 0.0).astype(np.float32)


def camera_rotations(rng, n):
    return sc.expmap(_unit(rng, n) * rng.uniform(0.3, 2.8, size=(n, 1)))


def group_lists(sizes=GROUP_SIZES, seed=0):
    """(group (M,), pair (M,), ref_pair (9,)) int32 of one scene: the cameras of each group in ascending order.  Groups of 8 see cameras
    0 .. 7; the group of 3 sees 3, 5 and 8 -- camera 8 never meets the reference camera 0, its d stays unknown; the others draw from
    0 .. 7, the reference camera among them in two groups of three."""
    rng = np.random.RandomState(seed + 50)
    group, pair = [], []
    for g, n in enumerate(sizes):
        if n == 8:
            cams = list(range(8))
        elif n == 3:
            cams = [3, 5, 8]
        else:
            cams = sorted(rng.choice(8, size=n, replace=False).tolist())
            if g % 3 != 2 and 0 not in cams:
                cams[0] = 0
        group += [g] * n
        pair += cams
    return np.array(group, np.int32), np.array(pair, np.int32), np.zeros(N_CAMS, np.int32)


def table_case(seed=4):
    """a dict: table (96,240) float32, order (70,), group, pair, ref_pair int32 -- the positions' records scattered over the rows by a
    non-monotone permutation, the 26 rows nobody lists unrefined (all zero) and in between --, E (9,3,3) the planted camera rotations, rel
    (9,4) float32 their planted d (camera 8: unknown) -- what the fusion tests pass to the kernel, so that the branch conditions can be
    met while the views are drawn -- and the outliers asked for, {first position of the group: (view, joint)}"""
    rng = np.random.RandomState(seed + 200)
    group, pair, ref_pair = group_lists(seed=seed)
    order = rng.permutation(N_ROWS)[:M].astype(np.int32)
    assert (np.diff(order) < 0).any() and (np.diff(order) > 0).any()
    E = camera_rotations(rng, N_CAMS)
    rel = planted_rel(E, np.arange(N_CAMS) != 8)
    x6d, outliers, at = [], {}, 0
    for g, n in enumerate(GROUP_SIZES):
        out = None
        if n >= 3 and g % 2 == 0:
            out = (int(rng.randint(n)), int(rng.choice([1, 4, 5, 7, 8, 9])))
            outliers[at] = out
        x6d.append(group_views(rng, pair[at:at + n], E, rel, outlier=out))
        at += n
    x6d = np.concatenate(x6d).astype(np.float32)
    table = np.zeros((N_ROWS, ROW), dtype=np.float32)
    table[order, 0:72] = rng.normal(size=(M, 72))                       # the axis-angle part: the kernels do not read it
    table[order, 72:216] = x6d.reshape(M, 144)
    table[order, 216:229] = rng.normal(size=(M, 13))
    table[order[0], 216], table[order[1], 217] = -0.0, -0.0             # signed zeros: a group of one keeps them
    table[order, 229] = 1.0
    table[order, 230:237] = rng.uniform(size=(M, 7))
    return {'table': table, 'order': order, 'group': group, 'pair': pair, 'ref_pair': ref_pair, 'E': E, 'rel': rel, 'outliers': outliers}


def positions_of(table, order):
    """(x6d (M,24,6), betas (M,10)) float32 in position order"""
    rows = table[order]
    return rows[:, 72:216].reshape(-1, 24, 6), rows[:, 216:226]


def yardstick(x6d, betas, group, pair, rel, max_deg, valid=None, check=True):
    """(float64 result, distances of the float32 result from it, the float32 result); `check`: the branch conditions hold"""
    chm = cos_half(max_deg)
    margins = []
    r64 = fuse(x6d, betas, group, pair, rel, chm, np.float64, valid, margins)
    if check:
        assert_branches(margins)
    r32 = fuse(x6d, betas, group, pair, rel, chm, np.float32, valid)
    assert np.array_equal(r32['taken'], r64['taken']) or not check
    return r64, distances(r32, r64), r32


PLANTED = dict(frames=200, cams=4, sigma_deg=5.0, replaced_view=2, replaced_share=0.3)


def planted_case(seed=11, replaced=False):
    """the planted-truth case: 200 frames x 4 cameras = 800 rows in (frame, camera) order; world rotations W (200,24,3,3), camera
    rotations E (4,3,3); view v of frame f shows E_v W_0 N and W_j N with N a rotation by |N(0, 5 deg)| about a random axis, independent
    per (frame, view, joint).  `replaced`: view 2 is a random rotation at 30 % of the (frame, body joint) pairs, `bad` (200, 24) bool.
    Exactly orthonormal 6-D values, rounded to float32."""
    rng = np.random.RandomState(seed)
    G, V = PLANTED['frames'], PLANTED['cams']
    W = sc.expmap(_unit(rng, G * 24) * rng.uniform(0, np.pi, size=(G * 24, 1))).reshape(G, 24, 3, 3)
    E = camera_rotations(rng, V)
    ang = np.abs(rng.normal(size=(G * V * 24, 1))) * np.radians(PLANTED['sigma_deg'])
    N = sc.expmap(_unit(rng, G * V * 24) * ang).reshape(G, V, 24, 3, 3)
    R = W[:, None] @ N
    R[:, :, 0] = E[None] @ R[:, :, 0]
    bad = np.zeros((G, 24), bool)
    if replaced:
        bad[:, 1:] = rng.uniform(size=(G, 23)) < PLANTED['replaced_share']
        R[:, PLANTED['replaced_view']][bad] = sc.expmap(_unit(rng, int(bad.sum())) * rng.uniform(0, np.pi, size=(int(bad.sum()), 1)))
    x6d = sc.to_6d(R).reshape(G * V, 24, 6).astype(np.float32)
    table = np.zeros((G * V, ROW), dtype=np.float32)
    table[:, 72:216], table[:, 229] = x6d.reshape(G * V, 144), 1.0
    table[:, 216:226] = rng.normal(size=(G * V, 10))
    return {'table': table, 'order': np.arange(G * V, dtype=np.int32), 'group': np.repeat(np.arange(G), V).astype(np.int32),
            'pair': np.tile(np.arange(V), G).astype(np.int32), 'ref_pair': np.zeros(V, np.int32), 'W': W, 'E': E, 'bad': bad, 'x6d': x6d}


def planted_errors(case, x6d_out, dropped=None):
    """what the planted-truth test asserts, of fused 6-D rows (800,24,6): the mean body-rotation error of the single views and of the
    fused pose (view 0's row: every member holds the same body), in degrees; with replaced pairs the same over those pairs only, the
    clean single views' mean there, and the share of them `dropped` (800,) accounts for"""
    G, V = PLANTED['frames'], PLANTED['cams']
    W, bad = case['W'], case['bad']
    single = rot_angle_deg(rot6d(case['x6d']).reshape(G, V, 24, 3, 3), W[:, None])[:, :, 1:]
    fused = rot_angle_deg(rot6d(x6d_out).reshape(G, V, 24, 3, 3)[:, 0], W)[:, 1:]
    out = {'single': float(single.mean()), 'fused': float(fused.mean())}
    if bad.any():
        b = bad[:, 1:]
        clean = np.delete(single, PLANTED['replaced_view'], 1)
        out.update(single_clean=float(clean.mean()), fused_bad=float(fused[b].mean()), fused_clean=float(fused[~b].mean()))
        if dropped is not None:
            d = np.asarray(dropped).reshape(G, V)
            out['flagged'] = float(np.minimum(d[:, PLANTED['replaced_view']], b.sum(1)).sum() / b.sum())
            out['dropped_elsewhere'] = int(np.delete(d, PLANTED['replaced_view'], 1).sum())
    return out


def planted_reference(seed=11):
    """the float64 restatement on the planted cases, with the builder's own assertions (DESIGN.md section 3h has the figures): the relative rotations
    within 1.5 degrees of E_ref E_c^T; fused / single body error <= 0.65; with replaced views, the trimmed error there <= the clean single
    views' mean, the plain mean's not, and the replaced view dropped in >= 95 % of the pairs.  Returns the figures."""
    case = planted_case(seed)
    count, mean = accumulate(case['x6d'], case['group'], case['pair'], case['ref_pair'])
    rel, residual = solve(count, mean, case['ref_pair'])
    truth = quats(sc.to_6d(case['E'][0][None] @ case['E'].transpose(0, 2, 1)))
    rel_err = np.degrees(2 * np.arccos(np.clip(np.abs(qdot(rel.astype(np.float64), truth)), 0, 1)))
    limit = 3 * PLANTED['sigma_deg'] * np.sqrt(2.0 / PLANTED['frames'])
    assert count.tolist() == [0, 200, 200, 200] and rel_err.max() <= limit, (count, rel_err)
    figures = {'rel': rel, 'rel_err_deg': rel_err, 'residual_deg': residual, 'limit_deg': limit}
    betas = case['table'][:, 216:226]
    margins = []
    r = fuse(case['x6d'], betas, case['group'], case['pair'], rel, cos_half(30.0), margins=margins)
    assert_branches(margins, cost=False)
    figures['clean'] = planted_errors(case, r['x6d'])
    assert figures['clean']['fused'] <= 0.65 * figures['clean']['single'], figures['clean']
    bad_case = planted_case(seed, replaced=True)
    exempt = lambda first, j: bool(bad_case['bad'][first // PLANTED['cams'], j])
    for max_deg in (30.0, 0.0):
        margins = []
        r = fuse(bad_case['x6d'], betas, bad_case['group'], bad_case['pair'], rel, cos_half(max_deg), margins=margins)
        assert_branches(margins, exempt=exempt, cost=False)
        figures[f'replaced_{max_deg:g}'] = planted_errors(bad_case, r['x6d'], r['dropped'])
    t, p = figures['replaced_30'], figures['replaced_0']
    assert t['fused_bad'] <= t['single_clean'] < p['fused_bad'] and t['flagged'] >= 0.95, (t, p)
    return figures


# ---- a dataset directory with a camera rig ----------------------------------------------------------------------------------
def logmap(R):
    """(n,3,3) -> (n,3) float64 axis-angle, angle in [0, pi]"""
    q = quats(sc.to_6d(np.asarray(R, np.float64)))
    q = np.where(q[:, :1] < 0, -q, q)
    n = np.linalg.norm(q[:, 1:], axis=1, keepdims=True)
    return np.where(n > 0, q[:, 1:] / np.where(n > 0, n, 1.0), 0.0) * 2 * np.arctan2(n, q[:, :1])


def rig_dataset(seed=5):
    """(paths, orient (40,3), pose (40,69)) float32 axis-angle start poses of 40 samples in a shuffled file order: scene `Walking 1` with
    cameras 1 - 4 over frames 5 .. 30 (camera 3 misses frames 10 and 25), scene `Eating 2` with four cameras over frames 2 .. 8 and camera
    1 alone at frame 10, and a stray path without imageSequence.  The views of one instant show one body: per joint a world rotation, seen
    through the camera's rotation at joint 0; one view of each instant carries no noise, the others 12 - 16 degrees about mutually
    orthogonal axes -- the quiet view stays the medoid by a margin that two refinement iterations do not eat."""
    rng = np.random.RandomState(seed)
    rows = [('Walking 1', str(c), f) for f in range(5, 35, 5) for c in range(1, 5) if not (c == 3 and f in (10, 25))]
    rows += [('Eating 2', str(c), f) for f in (2, 4, 6, 8) for c in range(1, 5)] + [('Eating 2', '1', 10), None]
    assert len(rows) == 40
    E = {(scene, str(c)): camera_rotations(rng, 1)[0] for scene in ('Walking 1', 'Eating 2') for c in range(1, 5)}
    aa = np.zeros((40, 24, 3))
    instants = {}
    for i, r in enumerate(rows):
        if r is not None:
            instants.setdefault((r[0], r[2]), []).append(i)
    for members in instants.values():
        V = len(members)
        quiet = rng.randint(V)
        for j in range(24):
            W = sc.expmap(rng.normal(scale=0.3, size=(1, 3)))[0]
            frame = np.linalg.qr(rng.normal(size=(3, 3)))[0]
            k = 0
            for v, i in enumerate(members):
                R = W
                if v != quiet:
                    R = W @ sc.expmap(frame[:, k % 3][None] * np.radians(rng.uniform(12.0, 16.0)))[0]
                    k += 1
                if j == 0:
                    R = E[rows[i][:2]] @ R
                aa[i, j] = logmap(R[None])[0]
    aa[39] = rng.normal(scale=0.3, size=(24, 3))
    perm = rng.permutation(40)
    paths = ['/data/elsewhere/000001.jpg' if r is None else f'/data/h36m/S9/{r[0]}/imageSequence/{r[1]}/img_{r[2]:06d}.jpg' for r in rows]
    paths = [paths[i] for i in perm]
    aa = aa[perm].astype(np.float32)
    return paths, aa[:, 0], aa[:, 1:].reshape(40, 69)
