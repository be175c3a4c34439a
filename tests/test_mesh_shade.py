"""The shaded mesh views of the fit report on the CPU: the vertex-face adjacency, the known answers of the host restatement
(tests/mesh_shade_cases.py) that the GPU tests measure against, report.side_view, the `--fit_report_mesh` flag check and the driver's
ordering with the flag under the recording stand-in (tests/driver_standin.py)."""
import functools
import importlib

import numpy as np
import pytest
import torch

import driver_standin as ds
import mesh_shade_cases as msc
from conftest import PKG_NAME

F32, F64 = np.float32, np.float64


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


# ---- adjacency ----
def _check_adjacency(faces, n_verts):
    offset, adj = _mod('report').vertex_face_adjacency(faces, n_verts)
    F = len(faces)
    assert offset.dtype == np.int32 and adj.dtype == np.int32 and offset.shape == (n_verts + 1,) and adj.shape == (3 * F,)
    assert offset[0] == 0 and offset[-1] == 3 * F and (np.diff(offset) >= 0).all()
    assert np.array_equal(np.bincount(adj, minlength=F), np.full(F, 3))              # every face exactly three times
    lists = msc.adjacency_lists(faces, n_verts)
    for v in range(n_verts):
        mine = adj[offset[v]:offset[v + 1]].tolist()
        assert mine == sorted(mine) == lists[v], v
    return offset, adj


def test_adjacency_of_a_tetrahedron_a_fan_and_the_body(smpl_model_np):
    offset, _ = _check_adjacency(msc.tetrahedron()[1], 4)
    assert np.diff(offset).tolist() == [3, 3, 3, 3]
    verts, faces = msc.fan(70)
    offset, adj = _check_adjacency(faces, len(verts))
    assert np.diff(offset).tolist() == [70] + [2] * 70 and adj[:70].tolist() == list(range(70))
    offset, _ = _check_adjacency(smpl_model_np['faces'], 6890)
    assert np.diff(offset).max() == 82 and np.diff(offset).min() >= 1               # the synthetic body's two poles


def test_adjacency_isolated_vertices_have_empty_lists():
    faces = msc.tetrahedron()[1] + 1                        # vertices 0 and 5 .. 6 belong to no face
    offset, adj = _check_adjacency(faces, 7)
    assert np.diff(offset).tolist() == [0, 3, 3, 3, 3, 0, 0]


def test_adjacency_is_cached_and_refuses_bad_faces():
    report = _mod('report')
    faces = msc.tetrahedron()[1]
    assert report.vertex_face_adjacency(faces, 4)[1] is report.vertex_face_adjacency(faces.copy(), 4)[1]
    assert report.vertex_face_adjacency(torch.from_numpy(faces), 4)[1] is report.vertex_face_adjacency(faces, 4)[1]
    with pytest.raises(ValueError):
        report.vertex_face_adjacency(faces, 3)
    with pytest.raises(ValueError):
        report.vertex_face_adjacency(faces.astype(np.float32), 4)
    with pytest.raises(ValueError):
        report.vertex_face_adjacency(faces[:, :2], 4)


# ---- the restatement's own known answers ----
@pytest.mark.parametrize('dtype', [F32, F64])
def test_restatement_regular_tetrahedron(dtype):
    verts, faces = msc.tetrahedron()
    n = msc.vertex_normals_ref(verts[None], faces, dtype)[0]
    want = verts.astype(F64) / np.sqrt(3.0)
    assert np.abs(n - want).max() <= (1e-15 if dtype is F64 else 2e-7)
    inward = msc.vertex_normals_ref(verts[None], faces[:, ::-1], dtype)[0]           # the other winding: -v / |v|
    assert np.array_equal(inward, -n)


@pytest.mark.parametrize('dtype', [F32, F64])
def test_restatement_flat_quad_and_isolated_vertex(dtype):
    verts, faces = msc.quad()
    verts = np.concatenate([verts, [[3, 3, 3]]]).astype(F32)                         # vertex 4 belongs to no face
    n = msc.vertex_normals_ref(verts[None], faces, dtype)[0]
    assert np.array_equal(n[:4], np.tile([0, 0, 1], (4, 1))) and np.array_equal(n[4], [0, 0, 0])


@pytest.mark.parametrize('dtype', [F32, F64])
def test_restatement_depth_of_a_fronto_parallel_triangle_is_its_z(dtype):
    S = 16
    verts = np.array([[[-0.1, -0.1, 0.25], [0.12, -0.1, 0.25], [0.0, 0.13, 0.25]]], dtype=F32)
    faces = np.array([[0, 1, 2]], dtype=np.int32)
    cam = np.array([[0.0, 0.0, 30.0]], dtype=F32)
    normals = msc.vertex_normals_ref(verts, faces, F32).astype(F32)
    p2f = np.full((1, S, S), -1, dtype=np.int32)
    p2f[0, 6:10, 6:10] = 0
    out = msc.shade_ref(verts, normals, faces, cam, p2f, dtype)
    drawn = p2f[0] >= 0
    assert out['status'] == 0 and np.abs(out['depth'][0][drawn] - 30.5).max() <= (1e-13 if dtype is F64 else 1e-5)
    assert (out['depth'][0][~drawn] == -1).all() and (out['normal'][0][~drawn] == 0).all() and (out['rgb'][0][~drawn] == 0).all()
    # the triangle faces the camera: |n . l| = 1 under the headlight, the base colour at full intensity
    assert np.abs(np.abs(out['normal'][0][drawn]) - [0, 0, 1]).max() <= 1e-6
    assert (out['rgb'][0][drawn] == np.floor(np.asarray(msc.COLOUR, dtype=F32).astype(F64) * 255 + 0.5).astype(np.uint8)).all()


def test_restatement_clip_and_status_bits():
    verts, normals, faces, cam, p2f = msc.scene(32, 1)
    p2f[0, 3, 3], p2f[0, 3, 4] = 2, 7                                                # an index >= F
    out = msc.shade_ref(verts, normals, faces, cam, p2f, F64)
    assert out['status'] == 1 and out['depth'][0, 3, 3] == -1 and (out['depth'][0][p2f[0] == 1] > 0).all()
    w = out['weights']
    assert (w >= 0).all() and (w <= 1).all() and np.abs(w.sum(-1) - 1).max() <= 1e-12
    assert w[0].min() == 0 and w[-1].min() == 0                                     # pixels (0,0) and (S-1,S-1): far outside, clipped
    assert 50 < (p2f[0] >= 0).sum() < 32 * 32 // 2 and (p2f[0] == 0).sum() > 20 and (p2f[0] == 1).sum() > 20
    assert np.abs(np.linalg.norm(out['normal'][0][p2f[0] == 0], axis=-1) - 1).max() <= 1e-12
    flat = verts.copy()
    flat[0, 3] = flat[0, 0]                                                          # face 1 = (0, 2, 3) collapses
    out = msc.shade_ref(flat, normals, faces, cam, msc.scene(32, 1)[4], F64)
    assert out['status'] == 2 and (out['depth'][0][msc.scene(32, 1)[4][0] == 1] == -1).all()


# ---- side_view ----
def _views(B=3, V=50, seed=2):
    g = torch.Generator().manual_seed(seed)
    verts = torch.randn(B, V, 3, generator=g) * 0.4
    cam = torch.randn(B, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, 40.0])
    return verts, cam


def test_side_view_four_quarter_turns_and_the_centroid():
    report = _mod('report')
    verts, cam = _views()
    flip = torch.tensor([-2.0, -2.0, 2.0])
    centre = (verts * flip + cam[:, None]).mean(1)
    v = verts
    for _ in range(4):
        v = report.side_view(v, cam)
        assert v.shape == verts.shape and v.dtype == verts.dtype
        assert ((v * flip + cam[:, None]).mean(1) - centre).abs().max().item() <= 1e-5          # turned about its own centroid
        assert torch.equal(v[..., 1], verts[..., 1])                                            # the axis is vertical
    assert (v - verts).abs().max().item() <= 1e-5
    # a quarter turn swaps the body's width and depth about the centroid, as seen by the camera
    d0 = (verts - verts.mean(1, keepdim=True)) * flip
    d1 = (report.side_view(verts, cam) - verts.mean(1, keepdim=True)) * flip
    assert (d1[..., 0] - d0[..., 2]).abs().max().item() <= 1e-5 and (d1[..., 2] + d0[..., 0]).abs().max().item() <= 1e-5
    # other angles compose
    twice = report.side_view(report.side_view(verts, cam, 45.0), cam, 45.0)
    assert (twice - report.side_view(verts, cam)).abs().max().item() <= 1e-5


def test_side_view_by_zero_is_the_identity_bit_for_bit():
    report = _mod('report')
    verts, cam = _views(seed=9)
    out = report.side_view(verts, cam, 0.0)
    assert out.data_ptr() != verts.data_ptr() and np.array_equal(out.numpy().view(np.uint32), verts.numpy().view(np.uint32))
    assert np.array_equal(report.side_view(verts, cam, 360.0).numpy().view(np.uint32), verts.numpy().view(np.uint32))
    with pytest.raises(ValueError):
        report.side_view(verts, cam[:2])
    with pytest.raises(ValueError):
        report.side_view(verts[0], cam)


# ---- the flag ----
def _with_args(flags, fn):
    argsmod = _mod('args')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(list(flags))
    try:
        return fn()
    finally:
        argsmod._LazyArgs._ns = saved


def test_check_flags_refuses_the_mesh_views_without_the_report(tmp_path):
    opt = _mod('optimize')
    assert _mod('args').get_args([]).fit_report_mesh is False
    with pytest.raises(ValueError, match='--fit_report_mesh needs --fit_report'):
        _with_args(['--silhouette', '--fit_report_mesh'], opt._check_flags)
    with pytest.raises(ValueError, match='--fit_report needs --silhouette'):
        _with_args(['--fit_report', str(tmp_path), '--fit_report_mesh'], opt._check_flags)
    _with_args(['--silhouette', '--fit_report', str(tmp_path), '--fit_report_mesh'], opt._check_flags)


# ---- the driver's ordering ----
SMALL = ('--batch_size', '6', '--inner_iters', '2', '--synthetic_batches', '2', '--silhouette')
MESH_ONLY = {'silhouette_pix_to_face', 'mesh_shade'}
# the calls of today's driver with SMALL + --fit_report, one outer batch, by name: what the flag must leave as it is
RENDER = ['find_joints_forward', 'silhouette_forward', 'project_joints', 'silhouette_compare']


class MeshEngine(ds.FakeEngine):
    def silhouette_pix_to_face(self):
        return ds.new(ds.record('silhouette_pix_to_face'), self.batch, self.sil, self.sil, dtype=torch.int32)


def mesh_shade(verts, cam, pix_to_face, faces, normals=None, image=None, normalize=None, background=0.0, **_):
    crc = ds.record('mesh_shade', [verts, cam, pix_to_face, normals, image], normalize=normalize, background=background, faces=tuple(faces.shape))
    return ds.new(crc, pix_to_face.shape[0], pix_to_face.shape[1], pix_to_face.shape[2], 3, dtype=torch.uint8)


@functools.lru_cache(maxsize=None)
def _run(flags):
    report = _mod('report')
    saved = ds.FakeEngine, report.mesh_shade
    ds.FakeEngine, report.mesh_shade = MeshEngine, mesh_shade
    try:
        return ds.run(list(flags))
    finally:
        ds.FakeEngine, report.mesh_shade = saved


@pytest.fixture(scope='module')
def out(tmp_path_factory):
    return tmp_path_factory.mktemp('mesh_steps')


def _name(line):
    return line.split()[1]


def _per_batch(log):
    starts = [i for i, l in enumerate(log) if _name(l) == 'set_batch_norm']
    ends = [i for i, l in enumerate(log) if _name(l) == 'read_back']
    assert len(starts) == len(ends) == 2
    return [log[s:e + 1] for s, e in zip(starts, ends)]


def test_each_render_is_forward_raster_faces_raster_faces_at_the_two_places(out):
    _, log = _run(SMALL + ('--fit_report', str(out / 'fit'), '--fit_report_mesh'))
    for lines in _per_batch(log):
        names = [_name(l) for l in lines]
        renders = [i for i, n in enumerate(names) if n == 'project_joints']
        assert len(renders) == 2
        for p in renders:
            assert names[p - 5:p + 1] == ['find_joints_forward', 'silhouette_forward', 'silhouette_pix_to_face', 'silhouette_forward',
                                          'silhouette_pix_to_face', 'project_joints']
            assert 'return_verts=True' in lines[p - 5]
            # the second rasterisation draws other vertices (the turned body) with the same camera
            assert lines[p - 4].split('crc=')[1] != lines[p - 2].split('crc=')[1]
        assert names.count('silhouette_pix_to_face') == 4
        before, after = renders
        term_on = next(i for i, l in enumerate(lines) if _name(l) == 'set_silhouette' and '[None' not in l)
        loop = names.index('refine_run')
        assert before < term_on < loop                                   # ahead of set_silhouette / refine_run
        assert after - 5 > names.index('find_joints_after_j_step')       # behind the joints after the J step
        readers = [l for l in lines[after + 1:] if _name(l) in ('find_joints_after_j_step', 'refine_aux_losses')
                   or (_name(l) == 'refine_run' and 'after_j_step=True' in l)]
        assert not readers                                               # nothing reads the engine's forward after them
        # the pictures: per render the front view, then the side view over grey, of the kept poses
        shades = [l for l in lines if _name(l) == 'mesh_shade']
        assert len(shades) == 4 and all('(6, 6890, 3)' in l and '(6, 224, 224):int32' in l for l in shades)
        assert ['background=0.25' in l for l in shades] == [False, True, False, True]


def test_without_the_flag_the_call_sequence_is_todays(out):
    strip = lambda lines: [l.split(' ', 1)[1] for l in lines]
    _, plain = _run(SMALL + ('--fit_report', str(out / 'fit_plain')))
    _, mesh = _run(SMALL + ('--fit_report', str(out / 'fit'), '--fit_report_mesh'))
    assert not [l for l in plain if _name(l) in MESH_ONLY]
    # today's shape of a render and of the report's tail, by name
    for lines in _per_batch(plain):
        names = [_name(l) for l in lines]
        for p in (i for i, n in enumerate(names) if n == 'project_joints'):
            assert names[p - 2:p + 2] == RENDER
        assert names.count('silhouette_forward') == 3 and names.count('fit_overlay') == 2       # the synthetic mask's, and the two renders
    # the flag's own lines taken out, the run without it is left line for line (names, shapes, scalars and the CRC of every argument)
    own = set()
    for i, l in enumerate(mesh):
        if _name(l) in MESH_ONLY:
            own.add(i)
        if _name(l) == 'silhouette_pix_to_face' and _name(mesh[i - 1]) == 'silhouette_forward' and _name(mesh[i - 2]) == 'silhouette_pix_to_face':
            own.add(i - 1)                                                                      # the side view's rasterisation
    assert len(own) == 2 * (4 + 2 + 4) and strip(l for i, l in enumerate(mesh) if i not in own) == strip(plain)


def test_mesh_pictures_are_written_beside_the_overlays(out):
    import os
    import fit_report_cases as frc
    _run(SMALL + ('--fit_report', str(out / 'fit'), '--fit_report_mesh'))
    names = sorted(os.listdir(out / 'fit'))
    assert names == sorted(f'b{b:04d}_p{p:05d}_{w}{m}.png' for b in range(2) for p in range(6) for w in ('before', 'after') for m in ('', '_mesh'))
    assert frc.read_png(str(out / 'fit' / 'b0001_p00005_after_mesh.png'))[0].shape == (224, 448, 3)
    assert frc.read_png(str(out / 'fit' / 'b0001_p00005_after.png'))[0].shape == (224, 224, 3)
