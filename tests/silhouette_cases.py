"""Silhouette rasteriser away from the centred body: scenes, a float64 rasteriser with margins, float64 alpha.

Host only (numpy, torch on the CPU).  tests/test_silhouette_cases.py pins this comparator against the fp32 oracle
(oracle/silhouette_port.py); tests/test_gpu_silhouette_edges.py holds the HIP kernels (csrc/sil.hip) to it.

raster64 restates the semantics at the top of oracle/silhouette_port.py in float64 on the fp32 projected vertices AS GIVEN:
covered iff all three barycentric coordinates of the pixel centre are > 0, pz >= 0, |area| > 1e-8; a face whose largest Z is
negative is culled; nearest pz wins, ties -> lowest face index; non-finite faces are dropped.  A pixel is AMBIGUOUS when a
float64 margin says an fp32 evaluation may legitimately decide otherwise:
  * some candidate face has a barycentric coordinate within its margin of 0,
  * the two nearest hits are within their depth tolerances of each other (identical faces excepted: bit-identical inputs give
    bit-identical depths in any arithmetic, and the lowest index wins),
  * a candidate's pz is within its depth tolerance of 0,
  * a candidate's |area| is within 10 % of 1e-8.
The margin of a coordinate is max(tau_w, e), e = 8 * 2^-24 * (|P1| + |P2|) / |area| + |w| * (the same for the area): the coordinate
is the edge function (p - a) x (b - a) = P1 - P2 over the area, each product carries three roundings of 2^-24 and the difference
one more (4 * 2^-24 in all; doubled).  e scales with the face's NDC magnitude over its size: 1e-6 for a one-pixel face of the
body, where tau_w = 1e-4 (a hundredth of a pixel of a 100-pixel face) governs, but 1e-3 and more for a face that straddles Z = 0
(NDC of 1e3 .. 1e7), which no fixed threshold explains.  The reference corner of each edge function is the one of
oracle/silhouette_port.py (pytorch3d's): an evaluation that anchors all three coordinates at one corner is held to the same
margins.  Depth tolerance of a candidate: tau_z * |pz| + sum_k e_k |z_k|.
"""
from __future__ import annotations

import functools
import importlib

import numpy as np
import torch

import oracle
from conftest import PKG_NAME
from oracle import silhouette_port as sp

V = 6890
MAX_FACES = 14336
TAU_W = 1e-4
TAU_Z = 1e-5
EPS23 = 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------------
# float64 rasteriser with margins
# ---------------------------------------------------------------------------------------------------------------------
def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def face_scale(ndc: np.ndarray, faces: np.ndarray):
    """per face (float64): signed area (edge function), M = max(1, max |ndc|), L = largest coordinate extent, finite flag"""
    x, y, z = (np.asarray(ndc[:, k], dtype=np.float64) for k in range(3))
    fx, fy, fz = x[faces], y[faces], z[faces]
    finite = np.isfinite(fx).all(1) & np.isfinite(fy).all(1) & np.isfinite(fz).all(1)
    fx, fy = np.where(finite[:, None], fx, 0.0), np.where(finite[:, None], fy, 0.0)
    area = _edge(fx[:, 2], fy[:, 2], fx[:, 0], fy[:, 0], fx[:, 1], fy[:, 1])
    M = np.maximum(1.0, np.maximum(np.abs(fx).max(1), np.abs(fy).max(1)))
    L = np.maximum(fx.max(1) - fx.min(1), fy.max(1) - fy.min(1))
    return area, M, L, finite


def raster64(ndc: np.ndarray, faces: np.ndarray, S: int, tau_w: float = TAU_W, tau_z: float = TAU_Z, return_candidates: bool = False,
             chunk_pairs: int = 3_000_000):
    """(pix_to_face (S,S) int32, ambiguous (S,S) bool) for one mesh; with return_candidates also (pix, face) of every candidate
    (sorted by pixel): the faces float64 allows an fp32 rasteriser to pick at that pixel."""
    faces = np.asarray(faces, dtype=np.int64)
    x, y, z = (np.asarray(ndc[:, k], dtype=np.float64) for k in range(3))
    area, M, L, finite = face_scale(ndc, faces)
    fx, fy, fz = x[faces], y[faces], z[faces]
    absa = np.abs(area)
    with np.errstate(invalid='ignore'):
        ok = finite & (absa > 0.9 * sp.K_EPS) & (fz.max(1) >= 0)
    fxo, fyo = np.where(ok[:, None], fx, 0.0), np.where(ok[:, None], fy, 0.0)
    KU = 8 * 2.0 ** -24
    with np.errstate(all='ignore'):
        q1, q2 = (fx[:, 2] - fx[:, 0]) * (fy[:, 1] - fy[:, 0]), (fy[:, 2] - fy[:, 0]) * (fx[:, 1] - fx[:, 0])
        ra = np.where(ok, KU * (np.abs(q1) + np.abs(q2)) / np.maximum(absa, 1e-300), 0.0)      # relative error of the area itself
    near_eps = ok & (absa <= 1.1 * sp.K_EPS)
    # pixel ranges of the bounding boxes, one pixel of slack (near misses lie outside the box by less than margin * size)
    lo = lambda v: np.clip(np.ceil((S * (1 - v) - 1) / 2 - 1.0), 0, S).astype(np.int64)
    hi = lambda v: np.clip(np.floor((S * (1 - v) - 1) / 2 + 1.0), -1, S - 1).astype(np.int64)
    xi_lo, xi_hi, yi_lo, yi_hi = lo(fxo.max(1)), hi(fxo.min(1)), lo(fyo.max(1)), hi(fyo.min(1))
    nx, ny = np.maximum(xi_hi - xi_lo + 1, 0), np.maximum(yi_hi - yi_lo + 1, 0)
    cnt = np.where(ok, nx * ny, 0)
    recs = []
    order = np.nonzero(cnt)[0]
    csum = np.cumsum(cnt[order])
    start = 0
    while start < len(order):
        base = csum[start - 1] if start else 0
        stop = max(int(np.searchsorted(csum, base + chunk_pairs, side='right')), start + 1)
        fsel = order[start:stop]
        c = cnt[fsel]
        fid = np.repeat(fsel, c)
        k = np.arange(len(fid)) - np.repeat(np.cumsum(c) - c, c)
        xi = xi_lo[fid] + k % nx[fid]
        yi = yi_lo[fid] + k // nx[fid]
        px, py = 1 - (2 * xi + 1) / S, 1 - (2 * yi + 1) / S
        a, zs = area[fid], fz[fid]
        ws, es = [], []
        for k in range(3):                        # w_k = edge(p; v_{k+1}, v_{k+2}) / area, the oracle's reference corners
            i, j = (k + 1) % 3, (k + 2) % 3
            p1, p2 = (px - fx[fid, i]) * (fy[fid, j] - fy[fid, i]), (py - fy[fid, i]) * (fx[fid, j] - fx[fid, i])
            w = (p1 - p2) / a
            ws.append(w)
            es.append(KU * (np.abs(p1) + np.abs(p2)) / np.abs(a) + np.abs(w) * ra[fid])
        pz = ws[0] * zs[:, 0] + ws[1] * zs[:, 1] + ws[2] * zs[:, 2]
        tz = tau_z * np.abs(pz) + es[0] * np.abs(zs[:, 0]) + es[1] * np.abs(zs[:, 1]) + es[2] * np.abs(zs[:, 2])
        tws = [np.maximum(tau_w, e) for e in es]
        cand = (ws[0] > -tws[0]) & (ws[1] > -tws[1]) & (ws[2] > -tws[2]) & (pz >= -tz)
        hit = (ws[0] > 0) & (ws[1] > 0) & (ws[2] > 0) & (pz >= 0) & (absa[fid] > sp.K_EPS)
        shaky = ~hit | (ws[0] < tws[0]) | (ws[1] < tws[1]) | (ws[2] < tws[2]) | (pz <= tz) | near_eps[fid]
        recs.append((yi[cand] * S + xi[cand], fid[cand], hit[cand], shaky[cand], pz[cand], tz[cand]))
        start = stop
    p2f = -np.ones(S * S, dtype=np.int32)
    amb = np.zeros(S * S, dtype=bool)
    if not recs or sum(len(r[0]) for r in recs) == 0:
        out = (p2f.reshape(S, S), amb.reshape(S, S))
        return out + ((np.zeros(0, np.int64), np.zeros(0, np.int64)),) if return_candidates else out
    pix, fid, hit, shaky, pz, tz = (np.concatenate([r[i] for r in recs]) for i in range(6))
    # a candidate that is not a clean hit, or a hit near a threshold, makes its pixel ambiguous
    amb[pix[shaky]] = True
    hp, hf, hz, htz = pix[hit], fid[hit], pz[hit], tz[hit]
    o = np.lexsort((hf, hz, hp))                  # by pixel, nearest first, ties -> lowest face index
    hp, hf, hz, htz = hp[o], hf[o], hz[o], htz[o]
    first = np.nonzero(np.r_[True, hp[1:] != hp[:-1]])[0]
    p2f[hp[first]] = hf[first]
    # depth: every later hit of the pixel within the tolerances of the winner (identical faces excepted)
    win = np.repeat(first, np.diff(np.r_[first, len(hp)]))
    close = (hz - hz[win] <= htz + htz[win]) & (np.arange(len(hp)) != win)
    if close.any():
        ci, wi = np.nonzero(close)[0], win[close]
        same = ((fx[hf[ci]] == fx[hf[wi]]) & (fy[hf[ci]] == fy[hf[wi]]) & (fz[hf[ci]] == fz[hf[wi]])).all(1)
        amb[hp[ci[~same]]] = True
    out = (p2f.reshape(S, S), amb.reshape(S, S))
    if return_candidates:
        o = np.argsort(pix, kind='stable')
        out = out + ((pix[o], fid[o]),)
    return out


def is_candidate(cand, p2f_other: np.ndarray) -> np.ndarray:
    """(S,S) bool: the other rasteriser's face at each pixel is the background or one of float64's candidates there"""
    pix, fid = cand
    S2 = p2f_other.size
    got = p2f_other.reshape(-1).astype(np.int64)
    keys = np.unique(pix * (MAX_FACES + 1) + fid)
    q = np.arange(S2) * (MAX_FACES + 1) + np.maximum(got, 0)
    return ((got < 0) | np.isin(q, keys)).reshape(p2f_other.shape)


# ---------------------------------------------------------------------------------------------------------------------
# float64 alpha, nearest edge, tie flag, and the derived bound on an fp32 alpha
# ---------------------------------------------------------------------------------------------------------------------
def _seg_dist2(px, py, ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    t = np.where(l2 <= sp.K_EPS, 0.0, np.clip(((px - ax) * dx + (py - ay) * dy) / np.maximum(l2, sp.K_EPS), 0, 1))
    qx, qy = ax + t * dx, ay + t * dy
    return (px - qx) ** 2 + (py - qy) ** 2


def alpha64(ndc: np.ndarray, faces: np.ndarray, p2f: np.ndarray, S: int, k_delta: float = 8.0):
    """For the winning faces `p2f` (S,S): dict of (S,S) arrays -- alpha (float64; 0 on the background), dist, edge (index of the
    nearest edge, k -> k+1; -1 on the background), tie (the two nearest edges equidistant to 1e-3 relative) and bound, the
    derived bound on |alpha_fp32 - alpha|:
        0.25 * 1e4 * 2 sqrt(d) * delta + 1e-6,   delta = k_delta * 2^-23 * max(1, max |ndc| of the face)
    (0.25 / sigma = the steepest slope of the sigmoid; d = |p - q|^2 moves by 2 sqrt(d) |dq|; q = a + t (b - a) and p - q carry a
    few roundings of 2^-24 relative to the coordinates' magnitude)."""
    faces = np.asarray(faces, dtype=np.int64)
    x, y = np.asarray(ndc[:, 0], dtype=np.float64), np.asarray(ndc[:, 1], dtype=np.float64)
    flat = p2f.reshape(-1)
    pix = np.nonzero(flat >= 0)[0]
    out = dict(alpha=np.zeros(S * S), dist=np.zeros(S * S), edge=-np.ones(S * S, dtype=np.int64), tie=np.zeros(S * S, dtype=bool),
               bound=np.full(S * S, 1e-6))
    if len(pix):
        f = faces[flat[pix]]
        px, py = 1 - (2 * (pix % S) + 1) / S, 1 - (2 * (pix // S) + 1) / S
        d = np.stack([_seg_dist2(px, py, x[f[:, k]], y[f[:, k]], x[f[:, (k + 1) % 3]], y[f[:, (k + 1) % 3]]) for k in range(3)], 1)
        ds = np.sort(d, 1)
        dist = ds[:, 0]
        out['dist'][pix] = dist
        out['edge'][pix] = d.argmin(1)
        out['tie'][pix] = (ds[:, 1] - ds[:, 0]) < 1e-3 * np.maximum(ds[:, 0], 1e-30)
        with np.errstate(over='ignore'):
            out['alpha'][pix] = 1.0 / (1.0 + np.exp(-dist / sp.SIGMA))
        M = np.maximum(1.0, np.maximum(np.abs(x[f]).max(1), np.abs(y[f]).max(1)))
        out['bound'][pix] = 0.25 / sp.SIGMA * 2 * np.sqrt(dist) * k_delta * EPS23 * M + 1e-6
    return {k: v.reshape(S, S) for k, v in out.items()}


def needed_delta_constant(alpha32: np.ndarray, ref: dict, where: np.ndarray) -> float:
    """the smallest k_delta (in the bound of alpha64, built with k_delta = 8) that covers |alpha32 - alpha| on `where`"""
    err = np.abs(alpha32.astype(np.float64) - ref['alpha'])[where] - 1e-6
    slope = (ref['bound'][where] - 1e-6) / 8.0
    ok = slope > 0
    return float((err[ok] / slope[ok]).max()) if ok.any() and (err[ok] > 0).any() else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# scenes: (verts (b,6890,3) fp32, cam (b,3) fp32, faces (F,3) int32, S)
# ---------------------------------------------------------------------------------------------------------------------
def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


@functools.lru_cache(maxsize=None)
def _model_and_j():
    sm = _mod('smpl_model')
    from conftest import load_golden
    t = load_golden('j_regressor_triplets.npz')
    return sm.synthetic_smpl(1234), sm.j_regressor_from_triplets(t['rows'], t['cols'], t['vals'])


BODY_SEED = 71


@functools.lru_cache(maxsize=None)
def bodies():
    """the two synthetic bodies of every body scene: (pose6d (2,24,6), betas (2,10), cam0 (2,3), gt_j3d (2,17,3)) fp32 numpy"""
    model, J = _model_and_j()
    b = _mod('smpl_model').synthetic_batch(model, J, 2, seed=BODY_SEED)
    return tuple(np.asarray(b[k], dtype=np.float32) for k in ('pose6d', 'betas', 'cam', 'gt_j3d'))


@functools.lru_cache(maxsize=None)
def body_verts() -> np.ndarray:
    """(2,6890,3) fp32: the oracle's SMPL forward of the two bodies"""
    model, _ = _model_and_j()
    x6, betas, _, _ = bodies()
    smpl = oracle.OracleSMPL(model)
    R = oracle.rot6d_to_rotmat(torch.from_numpy(x6).reshape(-1, 6)).view(2, 24, 3, 3)
    return smpl(R[:, :1], R[:, 1:], torch.from_numpy(betas)).vertices.detach().numpy().astype(np.float32)


def body_faces() -> np.ndarray:
    return np.ascontiguousarray(np.asarray(_model_and_j()[0]['faces'], dtype=np.int32))


# cameras of the body scenes.  A camera shift c moves the body by f c / Z in NDC (+x is LEFT, +y is UP); shifts are stated in NDC
# so that both image sizes frame the body alike.  The body is about 0.45 NDC wide and 1.6 tall at the synthetic distance.
BODY_CAMS = {
    'centre': dict(shift=(0.0, 0.0)),
    'left': dict(shift=(0.93, 0.05)),
    'right': dict(shift=(-0.93, -0.05)),
    'top': dict(shift=(0.07, 1.0)),
    'bottom': dict(shift=(-0.07, -1.0)),
    'corner': dict(shift=(0.95, 0.9)),
    'off': dict(shift=(2.7, 0.3)),
    'third': dict(zdiv=3.0),
    'close_1p2': dict(z=1.2),
    'close_0p37': dict(z=0.37, poses=1),       # part of the body behind the camera, ~400 faces straddle Z = 0; one pose: the oracle is slow here
}
ALL_Z_POSITIVE = {k: k != 'close_0p37' for k in BODY_CAMS}


def body_cam(name: str, S: int) -> np.ndarray:
    """(2,3) fp32 camera of body scene `name` (for both bodies)"""
    spec = BODY_CAMS[name]
    cam = bodies()[2].copy()
    if 'shift' in spec:
        cam[:, 0] += np.float32(spec['shift'][0] * cam[:, 2] / (5000.0 / S))
        cam[:, 1] += np.float32(spec['shift'][1] * cam[:, 2] / (5000.0 / S))
    if 'zdiv' in spec:
        cam[:, 2] /= np.float32(spec['zdiv'])
    if 'z' in spec:
        cam[:, 2] = np.float32(spec['z'])
    return cam.astype(np.float32)


def body_scene(name: str, S: int, verts: np.ndarray = None):
    """body scene `name` at image size S; `verts` (2,6890,3) replaces the oracle's vertices (the GPU tests pass the HIP forward's)"""
    n = BODY_CAMS[name].get('poses', 2)
    v = body_verts() if verts is None else verts
    return np.ascontiguousarray(v[:n]), np.ascontiguousarray(body_cam(name, S)[:n]), body_faces(), S


# ---- hand-made scenes (S = 256).  cam = (0, 0, 2 * 5000 / 256) and verts.z = 0 give Z = 39.0625 = 2 f, so x_ndc = f (-2 x) / Z = -x
# exactly for coordinates of few mantissa bits (f = 625 / 32): pixel centres (odd multiples of 1/256) and edges can be placed exactly.
HS = 256
HCAM = np.array([[0.0, 0.0, 2 * 5000.0 / HS]], dtype=np.float32)
Z_ZERO = -5000.0 / HS            # verts.z that gives Z exactly 0
Z_BEHIND = -2 * 5000.0 / HS      # verts.z that gives Z = -39.0625 (NDC mirrored: x_ndc = +x)
PARK = (0.0, 0.0, 0.0)


def _hand(points: dict, faces, park=PARK, park2=None):
    """points: vertex index -> (x_ndc, y_ndc, verts_z); every other vertex is parked (alternating park / park2 if given)"""
    v = np.empty((1, V, 3), dtype=np.float32)
    v[0, :] = np.asarray(park, dtype=np.float32)
    if park2 is not None:
        v[0, 1::2] = np.asarray(park2, dtype=np.float32)
    for i, (xn, yn, vz) in points.items():
        v[0, i] = (-xn, -yn, vz)
    f = np.ascontiguousarray(np.asarray(faces, dtype=np.int32).reshape(-1, 3))
    assert set(f.reshape(-1).tolist()) <= set(points) | {PARK_VERTEX}
    return v, HCAM.copy(), f, HS


PARK_VERTEX = 3000               # a parked vertex used by filler faces (three times the same vertex: area 0)
BIG = {0: (-3.0, -1.5, 0.0), 6889: (3.0, -1.5, 0.0), 4000: (0.0, 4.5, 0.0)}      # contains the whole frame, edges >= 0.5 away
BIG_FACE = [0, 6889, 4000]


def centre(i: int) -> float:
    """NDC coordinate of pixel centre i at S = 256 (exact in fp32)"""
    return 1.0 - (2 * i + 1) / HS


def scene_big_triangle():
    return _hand(BIG, [BIG_FACE])


def scene_big_triangle_far_parked():
    """the parked vertices at NDC +-50: the pose's pixel box is far larger than the image"""
    return _hand(BIG, [BIG_FACE], park=(50.0, 50.0, 0.0), park2=(-50.0, -50.0, 0.0))


def scene_interpenetrating():
    """two frame-filling triangles in the planes z = +-0.1 x: the winner changes along a line"""
    pts, faces = {}, []
    for j, s in enumerate((0.1, -0.1)):
        ids = [10 + j, 3500 + j, 6000 + j]
        for i, (xn, yn, _) in zip(ids, BIG.values()):
            pts[i] = (xn, yn + 0.125 * j, s * -xn)
        faces.append(ids)
    return _hand(pts, faces)


TIE_PAIRS = ((5, 9000), (13 * 1024 + 5, 14000))     # (low, high) index of two identical faces; 13317 = thread 5's LAST register slot


def scene_identical_faces():
    """two pairs of identical faces among fillers of zero area: the lower index must win everywhere"""
    pts = {1: (0.9, -0.7, 0.0), 2: (0.1, -0.5, 0.0), 3: (0.45, 0.8, 0.0),
           4: (-0.1, 0.6, 0.0), 5: (-0.95, 0.7, 0.0), 6: (-0.5, -0.9, 0.0)}
    faces = np.full((14001, 3), PARK_VERTEX, dtype=np.int32)
    faces[TIE_PAIRS[0][0]] = faces[TIE_PAIRS[0][1]] = (1, 2, 3)
    faces[TIE_PAIRS[1][0]] = faces[TIE_PAIRS[1][1]] = (4, 5, 6)
    return _hand(pts, faces)


def scene_behind_camera():
    """face 0 has all three Z < 0 and lies, in image space, on top of the visible face 1: it must never appear"""
    vis = {1: (0.6, -0.6, 0.0), 2: (-0.7, -0.4, 0.0), 3: (0.1, 0.7, 0.0)}
    # (Z = -39.0625 mirrors the image: the NDC of these three are the NEGATIVES of the coordinates stated here)
    beh = {11: (-0.8, 0.8, Z_BEHIND), 12: (0.9, 0.5, Z_BEHIND), 13: (-0.2, -0.9, Z_BEHIND)}
    return _hand({**vis, **beh}, [[11, 12, 13], [1, 2, 3]])


def scene_visible_only():
    """scene_behind_camera without the culled face (same index for the visible one)"""
    v, cam, f, S = scene_behind_camera()
    f = f.copy()
    f[0] = PARK_VERTEX
    return v, cam, f, S


SLIVER_PIXEL = (127, 127)        # (row, col) whose centre (1/256, 1/256) the 2e-8 sliver covers


def scene_degenerate():
    """faces that cover nothing -- coincident vertices, collinear vertices, a sliver of |area| 0.5e-8 -- and a sliver of
    |area| 2e-8 laid over one pixel centre, which covers exactly that pixel"""
    c, w = centre(127), 2.0 ** -11            # 1/256
    h2, h05 = 2e-8 / (2 * w) / 2, 0.5e-8 / (2 * w) / 2
    pts = {1: (0.5, 0.5, 0.0), 2: (-0.5, -0.25, 0.0),                                       # coincident: (1, 1, 2)
           3: (-0.75, -0.75, 0.0), 4: (0.0, 0.0, 0.0), 5: (0.75, 0.75, 0.0),               # collinear, through pixel corners
           6: (-c - w, -c - h05, 0.0), 7: (-c + w, -c - h05, 0.0), 8: (-c, -c + h05, 0.0),   # 0.5e-8 over the centre of (128, 128)
           9: (c - w, c - h2, 0.0), 10: (c + w, c - h2, 0.0), 11: (c, c + h2, 0.0)}         # 2e-8 over the centre of (127, 127)
    return _hand(pts, [[1, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]])


EDGE_COL, EDGE_COL2, VERTEX_PIXEL = 230, 240, (60, 230)


def scene_edge_through_centres():
    """face 0: edge a-b runs exactly through the pixel centres of column 230 (rows 60 .. 120) and corner a sits exactly on the
    centre of (60, 230); face 1: edge c-a through the centres of column 240 (rows 140 .. 200).  Both edges start at corner a,
    relative to which the kernel forms its weights; the weights on them are exactly 0 in fp32 and float64, and > 0 is strict:
    those pixels are background.  (The faces are 200 pixels wide so that the pixels ON the edges stay under the ambiguity cap.)"""
    x0, x1, wd = centre(EDGE_COL), centre(EDGE_COL2), 200 * 2.0 / HS
    pts = {1: (x0, centre(60), 0.0), 2: (x0, centre(120) - 1.0 / 512, 0.0), 3: (x0 + wd, centre(90), 0.0),
           4: (x1, centre(140), 0.0), 5: (x1 + wd, centre(170) - 1.0 / 512, 0.0), 6: (x1, centre(200) - 1.0 / 512, 0.0)}
    return _hand(pts, [[1, 2, 3], [4, 5, 6]])


def scene_one_face():
    return _hand({7: (0.83, -0.41, 0.0), 8: (-0.37, -0.77, 0.0), 9: (-0.12, 0.66, 0.0)}, [[7, 8, 9]])


N_LAST_VISIBLE = 8


def scene_max_faces():
    """exactly MAX_FACES faces: the centred body's 13776, 552 of zero area, and 8 triangles over far-apart body vertices (the last
    register slot of the last threads is in use, and the last faces are visible)"""
    v, cam, f, S = body_scene('centre', HS)
    rng = np.random.RandomState(5)
    extra = np.full((MAX_FACES - len(f), 3), PARK_VERTEX, dtype=np.int32)
    extra[-N_LAST_VISIBLE:] = np.stack([rng.choice(V, 3, replace=False) for _ in range(N_LAST_VISIBLE)])
    return v[:1], cam[:1], np.ascontiguousarray(np.concatenate([f, extra])), S


def scene_big_triangle_nonfinite():
    """the big triangle plus faces that use a vertex with Z exactly 0 (NDC -inf, or NaN where X = Y = 0): they must change nothing"""
    pts = dict(BIG)
    pts[100] = (1.0, 1.0, Z_ZERO)           # -2 x / 0 -> +-inf
    pts[101] = (0.0, 0.0, Z_ZERO)           # 0 / 0 -> NaN
    pts[102] = (-0.5, 0.0, Z_ZERO)          # x -> inf, y -> NaN
    faces = [BIG_FACE, [0, 6889, 100], [100, 4000, 0], [6889, 100, 4000], [0, 101, 4000], [102, 0, 6889], [100, 101, 102]]
    return _hand(pts, faces)


HAND_SCENES = {
    'big_triangle': scene_big_triangle,
    'big_triangle_far_parked': scene_big_triangle_far_parked,
    'interpenetrating': scene_interpenetrating,
    'identical_faces': scene_identical_faces,
    'behind_camera': scene_behind_camera,
    'visible_only': scene_visible_only,
    'degenerate': scene_degenerate,
    'edge_through_centres': scene_edge_through_centres,
    'one_face': scene_one_face,
    'max_faces': scene_max_faces,
    'big_triangle_nonfinite': scene_big_triangle_nonfinite,
}


def check_expectation(name: str, p2f: np.ndarray, alpha: np.ndarray = None, others: dict = None):
    """the stated outcome of hand-made scene `name` for one rasteriser's pix_to_face (S,S) (and alpha, if given); `others`: name ->
    pix_to_face of the same rasteriser on the scenes this one is compared with"""
    if name in ('big_triangle', 'big_triangle_far_parked', 'big_triangle_nonfinite'):
        assert (p2f == 0).all(), (name, np.unique(p2f))
        if alpha is not None:
            assert (alpha == 1.0).all(), (name, float(alpha.min()))
    elif name == 'identical_faces':
        lows = [lo for lo, _ in TIE_PAIRS]
        assert set(np.unique(p2f).tolist()) == {-1, *lows}, np.unique(p2f)
        assert all((p2f == lo).sum() > 1000 for lo in lows)
    elif name == 'behind_camera':
        assert set(np.unique(p2f).tolist()) == {-1, 1}, np.unique(p2f)
        if others is not None:
            assert np.array_equal(p2f, others['visible_only'])
    elif name == 'degenerate':
        want = -np.ones_like(p2f)
        want[SLIVER_PIXEL] = 3
        assert np.array_equal(p2f, want), np.argwhere(p2f != want)
    elif name == 'edge_through_centres':
        assert (p2f[:131, EDGE_COL] == -1).all() and (p2f[:, EDGE_COL2] == -1).all()      # (face 1 crosses column 230 below row 140)
        assert p2f[VERTEX_PIXEL] == -1
        # ... and the neighbouring columns inside the faces are covered, row for row of the edges' spans
        assert (p2f[62:119, EDGE_COL - 1] == 0).all() and (p2f[142:199, EDGE_COL2 - 1] == 1).all()
        assert (p2f[:131, EDGE_COL + 1] == -1).all() and (p2f[:, EDGE_COL2 + 1] == -1).all()
    elif name == 'one_face':
        assert set(np.unique(p2f).tolist()) == {-1, 0} and (p2f == 0).sum() > 5000
    elif name == 'max_faces':
        assert (p2f >= MAX_FACES - N_LAST_VISIBLE).sum() > 100 and (p2f == MAX_FACES - 1).any(), p2f.max()


def pixel_box(ndc: np.ndarray, S: int):
    """(bx0, bx1, by0, by1): the pose's pixel box as the kernel forms it -- the projected vertices' box, clamped to the image"""
    with np.errstate(all='ignore'):
        x, y = ndc[:, 0].astype(np.float64), ndc[:, 1].astype(np.float64)
        lo = lambda v: int(np.clip(np.ceil(np.clip((S * (1 - v) - 1) / 2, -1, S)), 0, S))
        hi = lambda v: int(np.clip(np.floor(np.clip((S * (1 - v) - 1) / 2, -1, S)), -1, S - 1))
        return lo(np.nanmax(x)), hi(np.nanmin(x)), lo(np.nanmax(y)), hi(np.nanmin(y))


def strips(ndc: np.ndarray, S: int, zpix: int = 8960) -> int:
    """z-buffer strips the kernel sweeps for one pose: its pixel box in strips of as many box rows as fit `zpix` pixels"""
    bx0, bx1, by0, by1 = pixel_box(ndc, S)
    bw, bh = bx1 - bx0 + 1, by1 - by0 + 1
    return 0 if bw <= 0 or bh <= 0 else -(-bh // (zpix // bw))


def project32(verts: np.ndarray, cam: np.ndarray, S: int) -> np.ndarray:
    """(b,6890,3) fp32 projected vertices, the oracle's arithmetic (the kernels': the same operations in the same order)"""
    with np.errstate(all='ignore'):
        return sp.project_mesh(torch.from_numpy(verts), torch.from_numpy(cam), S).numpy()
