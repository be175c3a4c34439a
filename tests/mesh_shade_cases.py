"""Host restatement of the shaded mesh views and the inputs their tests share (tests/test_mesh_shade.py, tests/test_gpu_mesh_shade.py).

Written from the definitions include/jrr.h states for jrr_vertex_normals and jrr_mesh_shade -- pytorch3d's verts_normals_packed
(area-weighted sum of the face normals at a vertex, divided by max(|sum|, 1e-6)), the projection of the rasteriser, barycentrics from
the edge functions without perspective correction, clip_barycentric_coordinates, a two-sided directional light -- not from the kernels.
Every function takes the number format it evaluates in: float64 is the yardstick, and the distance of the float32 evaluation from it on
a test's own inputs sets that test's bound (3 x distance + 1e-7, the convention of DESIGN.md sections 3a, 3c, 3d)."""
import numpy as np

F32, F64 = np.float32, np.float64
COLOUR = (0.65, 0.74, 0.86)


def adjacency_lists(faces, n_verts):
    """per vertex the faces that name it, in ascending face index (a face that names a vertex twice is listed twice)"""
    lists = [[] for _ in range(n_verts)]
    for f, tri in enumerate(np.asarray(faces)):
        for v in tri:
            lists[int(v)].append(f)
    return lists


def vertex_normals_ref(verts, faces, dtype):
    """verts (B,V,3), faces (F,3) -> (B,V,3) in `dtype`: per vertex the sum over its faces, in ascending face index, of
    cross(p1 - p0, p2 - p0), divided by max(|sum|, 1e-6)"""
    v = np.asarray(verts).astype(dtype)
    faces = np.asarray(faces).astype(np.int64)
    B, V, _ = v.shape
    with np.errstate(all='ignore'):
        p0, p1, p2 = v[:, faces[:, 0]], v[:, faces[:, 1]], v[:, faces[:, 2]]
        e1, e2 = p1 - p0, p2 - p0
        cross = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1], e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                          e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], -1)
        lists = adjacency_lists(faces, V)
        s = np.zeros((B, V, 3), dtype=dtype)
        for k in range(max(len(l) for l in lists)):          # the k-th face of every vertex that has one: the list's order per vertex
            idx = np.array([i for i, l in enumerate(lists) if len(l) > k], dtype=np.int64)
            s[:, idx] = s[:, idx] + cross[:, np.array([lists[i][k] for i in idx], dtype=np.int64)]
        norm = np.sqrt((s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1]) + s[..., 2] * s[..., 2])
        return s / np.maximum(norm, dtype(1e-6))[..., None]             # torch's clamp(min=1e-6): a NaN stays a NaN


def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def shade_ref(verts, normals, faces, cam, p2f, dtype, image=None, normalize=None, colour=COLOUR, opacity=1.0, ambient=0.3,
              light=(0.0, 0.0, -1.0), background=0.0):
    """-> dict(rgb uint8 (B,S,S,3), depth (B,S,S), normal (B,S,S,3), status int, weights (n,3) of the drawn pixels): jrr_mesh_shade in
    `dtype`.  The scalar parameters pass through float32 first, as they cross the C boundary."""
    T = dtype
    v, nrm, cam = (np.asarray(a).astype(T) for a in (verts, normals, cam))
    faces, p2f = np.asarray(faces).astype(np.int64), np.asarray(p2f).astype(np.int64)
    B, S, _ = p2f.shape
    V, nF = v.shape[1], faces.shape[0]
    col = np.asarray(colour, dtype=F32).astype(T)
    lnorm = float(np.sqrt(sum(float(x) * float(x) for x in light)))
    l = np.asarray([float(x) / lnorm for x in light], dtype=F32).astype(T)
    op, amb = T(F32(opacity)), T(F32(ambient))
    with np.errstate(all='ignore'):
        if image is None:
            x = np.full((B, S, S, 3), F32(background), dtype=F32).astype(T)
        else:
            x = np.asarray(image, dtype=F32).astype(T)
            if normalize is not None:
                mean, std = (np.asarray(a, dtype=F32).astype(T).reshape(1, 3, 1, 1) for a in normalize)
                x = x * std + mean
            x = x.transpose(0, 2, 3, 1)
        bg = np.fmin(np.fmax(x, T(0)), T(1))
        value = bg.copy()                                    # what becomes the byte
        depth = np.full((B, S, S), T(-1))
        normal = np.zeros((B, S, S, 3), dtype=T)
        status = 0
        bb, ii, jj = np.nonzero(p2f >= 0)
        f = p2f[bb, ii, jj]
        inside = f < nF
        tri = faces[np.where(inside, f, 0)]
        inside &= ((tri >= 0) & (tri < V)).all(-1)
        if (~inside).any():
            status |= 1
        bb, ii, jj, tri = bb[inside], ii[inside], jj[inside], tri[inside]
        p = v[bb[:, None], tri]                              # (n,3 corners,3)
        n_k = nrm[bb[:, None], tri]
        c = cam[bb][:, None, :]
        X, Y, Z = T(-2) * p[..., 0] + c[..., 0], T(-2) * p[..., 1] + c[..., 1], T(2) * p[..., 2] + c[..., 2]
        foc = T(5000) / T(S)
        pu, pv = foc * X / Z, foc * Y / Z
        area = _edge(pu[:, 2], pv[:, 2], pu[:, 0], pv[:, 0], pu[:, 1], pv[:, 1])
        good = np.isfinite(pu).all(-1) & np.isfinite(pv).all(-1) & np.isfinite(Z).all(-1) & (np.abs(area) > T(F32(1e-8)))
        if (~good).any():
            status |= 2
        bb, ii, jj, pu, pv, Z, n_k, area = bb[good], ii[good], jj[good], pu[good], pv[good], Z[good], n_k[good], area[good]
        px, py = T(1) - (T(2) * jj.astype(T) + T(1)) / T(S), T(1) - (T(2) * ii.astype(T) + T(1)) / T(S)
        w = np.stack([_edge(px, py, pu[:, 1], pv[:, 1], pu[:, 2], pv[:, 2]) / area, _edge(px, py, pu[:, 2], pv[:, 2], pu[:, 0], pv[:, 0]) / area,
                      _edge(px, py, pu[:, 0], pv[:, 0], pu[:, 1], pv[:, 1]) / area], -1)
        w = np.fmax(w, T(0))
        w = w / np.fmax((w[:, 0] + w[:, 1]) + w[:, 2], T(F32(1e-5)))[:, None]
        depth[bb, ii, jj] = (w[:, 0] * Z[:, 0] + w[:, 1] * Z[:, 1]) + w[:, 2] * Z[:, 2]
        m = (w[:, 0, None] * n_k[:, 0] + w[:, 1, None] * n_k[:, 1]) + w[:, 2, None] * n_k[:, 2]
        n = m * np.asarray([-1, -1, 1], dtype=T)
        n = n / np.fmax(np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]), T(F32(1e-6)))[:, None]
        normal[bb, ii, jj] = n
        I = amb + (T(1) - amb) * np.abs((n[:, 0] * l[0] + n[:, 1] * l[1]) + n[:, 2] * l[2])
        value[bb, ii, jj] = np.fmin(np.fmax((op * col)[None, :] * I[:, None] + (T(1) - op) * bg[bb, ii, jj], T(0)), T(1))
        rgb = np.floor(value * T(255) + T(0.5)).astype(np.uint8)
    return dict(rgb=rgb, depth=depth, normal=normal, status=status, weights=w)


def bounds(ref32, ref64):
    """(max bound, mean bound) of one quantity: 3 x the float32 evaluation's distance from the float64 one + 1e-7"""
    d = np.abs(np.asarray(ref32, dtype=F64) - np.asarray(ref64, dtype=F64))
    return 3.0 * float(d.max()) + 1e-7, 3.0 * float(d.mean()) + 1e-7


# ---- shared meshes ----
def tetrahedron():
    """regular, centred at the origin, wound outward: every vertex normal is v / |v|"""
    verts = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=F32)
    faces = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)
    return verts, faces


def fan(valence=70, seed=3):
    """a cone: vertex 0 (the apex) in `valence` triangles over a wobbly rim, every rim vertex in two"""
    rng = np.random.RandomState(seed)
    ang = np.arange(valence) * (2 * np.pi / valence)
    rim = np.stack([np.cos(ang), np.sin(ang), 0.1 * rng.randn(valence)], 1)
    verts = np.concatenate([[[0.05, -0.02, 0.7]], rim]).astype(F32)
    faces = np.array([[0, 1 + k, 1 + (k + 1) % valence] for k in range(valence)], dtype=np.int32)
    return verts, faces


def quad():
    """two triangles in the plane z = 0.5, wound alike: the normal is (0,0,1) everywhere"""
    verts = np.array([[0, 0, 0.5], [1, 0, 0.5], [1, 1, 0.5], [0, 1, 0.5]], dtype=F32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    return verts, faces


def posed(verts, B, seed=5):
    """B poses of a mesh: seeded affine maps of it (pose 0 is the mesh itself)"""
    rng = np.random.RandomState(seed)
    out = [np.asarray(verts, dtype=F32)]
    for _ in range(B - 1):
        A = np.eye(3) + 0.3 * rng.randn(3, 3)
        out.append((verts @ A.T + 0.2 * rng.randn(3)).astype(F32))
    return np.stack(out)


def scene(S, B, seed=0):
    """The hand-made scene: V = 4, F = 2, a tilted quad about 0.7 NDC wide (the camera's depth follows the focal length 5000 / S), and a hand-written
    pix_to_face.  -> verts (B,4,3), normals (B,4,3) (unit, seeded, not the mesh's own: the interpolation has something to do), faces
    (2,3), cam (B,3), p2f (B,S,S) int32 holding -1, both faces at the pixels whose centres they cover, face 1 at pixel (0,0) and face
    0 at (S-1,S-1) -- centres far outside either face: the clip --, and nothing else."""
    rng = np.random.RandomState(100 * seed + S + B)
    faces = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    verts = np.stack([np.array([[-0.15, -0.12, 0.05], [0.16, -0.13, -0.04], [0.14, 0.15, 0.06], [-0.13, 0.14, -0.03]]) + 0.01 * rng.randn(4, 3)
                      for _ in range(B)]).astype(F32)
    z = 5000.0 / S * 0.45
    cam = (np.array([0.02, -0.03, z]) + np.array([0.02, 0.02, 0.02 * z]) * rng.randn(B, 3)).astype(F32)
    normals = rng.randn(B, 4, 3)
    normals = (normals / np.linalg.norm(normals, axis=-1, keepdims=True)).astype(F32)
    # which face covers which pixel centre, in float64 (the hand-written map; any map is a valid input of the operator)
    p2f = np.full((B, S, S), -1, dtype=np.int32)
    c = np.float64(1) - (2 * np.arange(S) + 1) / np.float64(S)
    px, py = np.meshgrid(c, c)                                  # px varies along the row (column index), py along the rows
    for b in range(B):
        X = -2.0 * verts[b, :, 0].astype(F64) + cam[b, 0]
        Y = -2.0 * verts[b, :, 1].astype(F64) + cam[b, 1]
        Z = 2.0 * verts[b, :, 2].astype(F64) + cam[b, 2]
        u, v = 5000.0 / S * X / Z, 5000.0 / S * Y / Z
        for f, (i0, i1, i2) in enumerate(faces):
            area = _edge(u[i2], v[i2], u[i0], v[i0], u[i1], v[i1])
            w = [_edge(px, py, u[a], v[a], u[c_], v[c_]) / area for a, c_ in ((i1, i2), (i2, i0), (i0, i1))]
            p2f[b][(w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)] = f
        p2f[b, 0, 0], p2f[b, S - 1, S - 1] = 1, 0
    return verts, normals, faces, cam, p2f


def background_image(B, S, seed=0):
    """(B,3,S,S) float32 in [0, 1] with exact 0, 1, and values outside planted"""
    rng = np.random.RandomState(31 * seed + S)
    image = rng.randint(0, 256, size=(B, 3, S, S)).astype(np.uint8).astype(F32) / F32(255)
    image[:, :, 1, 0], image[:, :, 1, 1], image[:, :, 1, 2], image[:, :, 1, 3] = 0.0, 1.0, -0.25, 1.5
    return image
