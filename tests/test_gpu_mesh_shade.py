"""The shaded mesh views on the GPU (pytest -m gpu): jrr_vertex_normals and jrr_mesh_shade against the float64 restatement of
tests/mesh_shade_cases.py, evaluated on the GPU's own pix_to_face; `--fit_report_mesh` through the driver; two gloo ranks.

There is no reference implementation (pytorch3d is absent, as for the rasteriser).  Every bound is computed in the test: 3 x the distance
of the restatement's float32 evaluation from its float64 evaluation on the test's own inputs + 1e-7, for the maximum and for the mean;
colour bytes are within 1 of the float64 restatement.  No pixel is left out of any comparison.

Shapes: V = 4 (fewer vertices than a wave) with B = 1, 3, 67 (B * V no multiple of the workgroup), a vertex of valence 70, the body
(V = 6890: 27 workgroups per pose); images of 4 x 4 (four quads), 32 x 32 (one workgroup), 64 x 64 and 224 x 224 (49 per pose).
"""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fit_report_cases as frc
import mesh_shade_cases as msc
from conftest import PKG_NAME, ROOT

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
F32, F64 = np.float32, np.float64
GUARD = 64                 # bytes on either side of a guarded output


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


@pytest.fixture(scope='module')
def smpl_hip(smpl_model_np):
    return _mod('smpl').SMPL(model=smpl_model_np).to(DEV)


def _guarded(n, dtype, fill):
    """a tensor of n elements with GUARD bytes of `fill` on either side -> (whole buffer, the view)"""
    g = GUARD // torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((n + 2 * g,), fill, dtype=dtype, device=DEV)
    return buf, buf[g:g + n]


def _guards_intact(buf, n, fill):
    g = (buf.numel() - n) // 2
    host = buf.cpu()
    return bool((host[:g] == fill).all() and (host[g + n:] == fill).all())


def _normals_gpu(verts, faces):
    """jrr_vertex_normals through the C ABI into a guarded output -> (B,V,3) numpy; asserts the guards"""
    report, lib_mod = _mod('report'), _mod('_lib')
    vd = T(np.ascontiguousarray(verts, dtype=F32)).to(DEV)
    B, V, _ = vd.shape
    f_dev, off_dev, adj_dev = report._device_mesh(faces, V, vd.device)
    buf, out = _guarded(B * V * 3, torch.float32, 12345.0)
    lib_mod.check(lib_mod.load().jrr_vertex_normals(lib_mod.ptr(vd), lib_mod.ptr(f_dev), lib_mod.ptr(off_dev), lib_mod.ptr(adj_dev), B, V,
                                                    f_dev.shape[0], lib_mod.ptr(out), lib_mod.stream_ptr(vd.device)), 'vertex_normals')
    torch.cuda.synchronize()
    assert _guards_intact(buf, B * V * 3, 12345.0)
    return out.view(B, V, 3).cpu().numpy()


def _held(name, got, ref32, ref64):
    """max and mean of |got - float64 restatement| against their yardsticks; prints the figures first"""
    err = np.abs(got.astype(F64) - ref64)
    bmax, bmean = msc.bounds(ref32, ref64)
    print(f'{name}: max {err.max():.3e} (bound {bmax:.3e})  mean {err.mean():.3e} (bound {bmean:.3e})')
    assert np.isfinite(err).all() and err.max() <= bmax and err.mean() <= bmean, name


# ---- 1. vertex normals ----
@pytest.mark.parametrize('B', [1, 3, 67])
def test_normals_of_a_tetrahedron(B):
    verts, faces = msc.tetrahedron()
    poses = msc.posed(verts, B)
    got = _normals_gpu(poses, faces)
    _held(f'tetrahedron B={B}', got, msc.vertex_normals_ref(poses, faces, F32), msc.vertex_normals_ref(poses, faces, F64))
    assert np.abs(got[0].astype(F64) - verts / np.sqrt(3.0)).max() <= 2e-7          # the regular one: v / |v|
    assert np.abs(np.linalg.norm(got.astype(F64), axis=-1) - 1).max() <= 1e-6


def test_normals_at_a_vertex_of_valence_70():
    verts, faces = msc.fan(70)
    poses = msc.posed(verts, 3)
    got = _normals_gpu(poses, faces)
    _held('fan of 70', got, msc.vertex_normals_ref(poses, faces, F32), msc.vertex_normals_ref(poses, faces, F64))
    assert np.array_equal(got, _mod('report').vertex_normals(T(poses).to(DEV), faces).cpu().numpy())       # the wrapper, its own allocation


def test_normals_isolated_vertex_and_zero_area_face():
    verts, faces = msc.quad()
    # vertex 4 belongs to no face; vertex 5 coincides with vertex 0 and belongs to the zero-area face (0, 5, 1) only
    verts = np.concatenate([verts, [[3, 3, 3]], verts[:1]]).astype(F32)
    faces = np.concatenate([faces, [[0, 5, 1]]]).astype(np.int32)
    poses = msc.posed(verts, 3)
    got = _normals_gpu(poses, faces)
    assert (got[:, 4] == 0).all() and (got[:, 5] == 0).all() and not np.signbit(got[:, 4]).any()
    _held('quad + isolated + zero area', got, msc.vertex_normals_ref(poses, faces, F32), msc.vertex_normals_ref(poses, faces, F64))
    assert np.abs(got[0, :4] - [0, 0, 1]).max() == 0


def test_normals_one_nan_vertex_poisons_its_neighbours_only():
    verts, faces = msc.fan(70)
    poses = msc.posed(verts, 3)
    clean = _normals_gpu(poses, faces)
    bad = poses.copy()
    bad[1, 5, 1] = np.nan
    got = _normals_gpu(bad, faces)
    touched = np.unique(faces[(faces == 5).any(1)])
    assert touched.tolist() == [0, 4, 5, 6]
    assert np.isnan(got[1, touched]).all()
    others = np.setdiff1d(np.arange(len(verts)), touched)
    assert np.array_equal(got[1, others], clean[1, others]) and np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2])


@pytest.fixture(scope='module')
def body(smpl_hip, smpl_model_np, j_h36m_np):
    """B = 3 poses of the synthetic body (synthetic_batch seed 31) rendered at 224: vertices, camera, the GPU's pix_to_face and normals,
    and the two evaluations of the normals' restatement -- computed once, read by the tests below, never written"""
    eng_mod, report = _mod('engine'), _mod('report')
    B = 3
    batch = _mod('smpl_model').synthetic_batch(smpl_model_np, j_h36m_np, B, seed=31)
    eng = eng_mod.RefineEngine(smpl_hip.device_model, B, flags=eng_mod.FLAG_SILHOUETTE | eng_mod.FLAG_KEEP_VERTS)
    eng.set_j_regressor(T(j_h36m_np))
    xd, bd, cd = (T(batch[k]).to(DEV).contiguous() for k in ('pose6d', 'betas', 'cam'))
    _, verts = eng.find_joints_forward(bd, x6d=xd, return_verts=True)
    eng.silhouette_forward(verts, cd)
    p2f = eng.silhouette_pix_to_face()
    faces = smpl_model_np['faces']
    normals = report.vertex_normals(verts, faces)
    v_np = verts.cpu().numpy()
    return dict(eng=eng, verts=verts, cam=cd, p2f=p2f, faces=faces, normals=normals, v_np=v_np,
                n32=msc.vertex_normals_ref(v_np, faces, F32), n64=msc.vertex_normals_ref(v_np, faces, F64))


def test_normals_of_the_body(body):
    got = _normals_gpu(body['v_np'], body['faces'])
    _held('body normals', got, body['n32'], body['n64'])
    assert np.abs(np.linalg.norm(got.astype(F64), axis=-1) - 1).max() <= 1e-5
    assert np.array_equal(got, body['normals'].cpu().numpy())                        # two calls give equal bits
    assert np.array_equal(got, _normals_gpu(body['v_np'], body['faces']))


# ---- 2. shade, hand-made scenes ----
VARIANTS = {'bare': {}, 'image': dict(image=True), 'normalised': dict(image=True, normalize=True), 'opacity': dict(image=True, opacity=0.6),
            'grey_sidelight': dict(background=0.25, light=(1.0, -1.0, -2.0), ambient=0.1, colour=(1.0, 0.5, 0.0)),
            'bad_index': dict(plant='index'), 'degenerate': dict(plant='degenerate', image=True)}


def _shade_case(S, B, variant):
    """the scene with the variant's plants -> (arrays of the scene, keyword arguments shared by the operator and the restatement)"""
    opts = dict(VARIANTS[variant])
    verts, normals, faces, cam, p2f = msc.scene(S, B)
    plant = opts.pop('plant', None)
    if plant == 'index':
        p2f[:, 0, 1], p2f[:, 1, 0] = 2, 2 ** 31 - 1           # F, and the largest int32
    if plant == 'degenerate':
        verts[B - 1, 3] = verts[B - 1, 0]                      # face 1 = (0, 2, 3) of the last pose collapses to a line
    kw = {k: opts[k] for k in ('opacity', 'background', 'light', 'ambient', 'colour') if k in opts}
    image = None
    if opts.get('image'):
        image = msc.background_image(B, S)
        if opts.get('normalize'):
            kw['normalize'] = _mod('data').SPIN_NORMALIZE
            mean, std = (np.asarray(v, dtype=F32).reshape(1, 3, 1, 1) for v in kw['normalize'])
            image = ((image - mean) / std).astype(F32)
    return (verts, normals, faces, cam, p2f, image), kw, plant


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('S', [4, 32])
def test_shade_hand_made_scene(S, B, variant):
    report = _mod('report')
    (verts, normals, faces, cam, p2f, image), kw, plant = _shade_case(S, B, variant)
    ref32 = msc.shade_ref(verts, normals, faces, cam, p2f, F32, image=image, **kw)
    ref64 = msc.shade_ref(verts, normals, faces, cam, p2f, F64, image=image, **kw)
    n = B * S * S
    buf, out = _guarded(n * 3, torch.uint8, 0xA5)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    dev = lambda a: None if a is None else T(np.ascontiguousarray(a)).to(DEV)
    args = (dev(verts), dev(cam), dev(p2f), faces)
    rgb, depth, nmap = report.mesh_shade(*args, normals=dev(normals), image=dev(image), out=out.view(B, S, S, 3), want_depth=True,
                                         want_normals=True, status=status, **kw)
    torch.cuda.synchronize()
    assert rgb.data_ptr() == out.data_ptr() and _guards_intact(buf, n * 3, 0xA5)
    assert depth.shape == (B, S, S) and nmap.shape == (B, S, S, 3) and depth.dtype == nmap.dtype == torch.float32
    assert status.item() == ref64['status'] == {None: 0, 'index': 1, 'degenerate': 2}[plant]
    depth, nmap, rgb = depth.cpu().numpy(), nmap.cpu().numpy(), rgb.cpu().numpy()
    _held(f'scene S={S} B={B} {variant} depth', depth, ref32['depth'], ref64['depth'])
    _held(f'scene S={S} B={B} {variant} normal', nmap, ref32['normal'], ref64['normal'])
    diff = np.abs(rgb.astype(np.int64) - ref64['rgb'].astype(np.int64))
    print(f'scene S={S} B={B} {variant}: {(diff != 0).sum()} of {diff.size} bytes differ from the float64 restatement, largest {diff.max()}')
    assert diff.max() <= 1
    # background pixels, the refused ones included: depth -1, normal 0, the background byte
    drawn = ref64['depth'] >= 0
    assert ((depth >= 0) == drawn).all() and (depth[~drawn] == -1).all() and (nmap[~drawn] == 0).all()
    if plant == 'index':
        assert not drawn[:, 0, 1].any() and not drawn[:, 1, 0].any()
    if plant == 'degenerate':
        assert not drawn[B - 1][p2f[B - 1] == 1].any() and drawn[B - 1][p2f[B - 1] == 0].all()
    # the pixels far outside their face (the clip): a unit normal, a depth within the face's own
    for i in (0, S - 1):
        if drawn[0, i, i]:
            Z = 2.0 * verts[0, :, 2].astype(F64) + cam[0, 2]
            assert abs(np.linalg.norm(nmap[0, i, i].astype(F64)) - 1) <= 1e-5 and Z.min() - 1e-3 <= depth[0, i, i] <= Z.max() + 1e-3
    assert np.abs(np.linalg.norm(nmap[drawn].astype(F64), axis=-1) - 1).max() <= 1e-5
    # the nullable outputs are optional: an allocation of its own, no maps, no status word -- the same bytes
    alone = report.mesh_shade(*args, normals=dev(normals), image=dev(image), **kw)
    assert torch.is_tensor(alone) and np.array_equal(alone.cpu().numpy(), rgb)
    only_depth = report.mesh_shade(*args, normals=dev(normals), image=dev(image), want_depth=True, **kw)
    assert only_depth[2] is None and np.array_equal(only_depth[1].cpu().numpy(), depth) and np.array_equal(only_depth[0].cpu().numpy(), rgb)


def test_shade_refuses_what_it_cannot_draw():
    report = _mod('report')
    verts, normals, faces, cam, p2f = msc.scene(32, 1)
    dev = lambda a: T(np.ascontiguousarray(a)).to(DEV)
    with pytest.raises(ValueError):
        report.mesh_shade(dev(verts), dev(cam), dev(p2f[:, :30, :30]), faces)         # 30: no multiple of 4
    with pytest.raises(ValueError):
        report.mesh_shade(dev(verts), dev(cam), dev(p2f).long(), faces)
    with pytest.raises(ValueError):
        report.mesh_shade(dev(verts), dev(cam), dev(p2f), faces, normalize=_mod('data').SPIN_NORMALIZE)
    with pytest.raises(ValueError):
        report.mesh_shade(dev(verts), dev(cam), dev(p2f), faces, light=(0, 0, 0))
    with pytest.raises(ValueError):
        report.mesh_shade(dev(verts), dev(cam)[:, :2], dev(p2f), faces)
    lib_mod = _mod('_lib')
    with pytest.raises(lib_mod.JrrError):                                               # the C boundary itself: a misaligned map
        odd = torch.zeros(32 * 32 + 1, dtype=torch.int32, device=DEV)[1:].view(1, 32, 32)
        report.mesh_shade(dev(verts), dev(cam), odd, faces)
    # normals computed by the operator when none are handed over
    own = report.mesh_shade(dev(verts), dev(cam), dev(p2f), faces)
    given = report.mesh_shade(dev(verts), dev(cam), dev(p2f), faces, normals=report.vertex_normals(dev(verts), faces))
    assert torch.equal(own, given)


# ---- 3. shade on rendered bodies ----
def _shade_body(body, verts, p2f):
    report = _mod('report')
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    normals = report.vertex_normals(verts, body['faces'])
    rgb, depth, nmap = report.mesh_shade(verts, body['cam'], p2f, body['faces'], normals=normals, want_depth=True, want_normals=True, status=status)
    return normals, rgb.cpu().numpy(), depth.cpu().numpy(), nmap.cpu().numpy(), status.item()


def _against_restatement(name, body, verts, normals, p2f, rgb, depth, nmap):
    a = (verts.cpu().numpy(), normals.cpu().numpy(), body['faces'], body['cam'].cpu().numpy(), p2f.cpu().numpy())
    ref32, ref64 = msc.shade_ref(*a, F32), msc.shade_ref(*a, F64)
    assert ref64['status'] == 0
    _held(f'{name} depth', depth, ref32['depth'], ref64['depth'])
    _held(f'{name} normal', nmap, ref32['normal'], ref64['normal'])
    diff = np.abs(rgb.astype(np.int64) - ref64['rgb'].astype(np.int64))
    print(f'{name}: {(diff != 0).sum()} of {diff.size} bytes differ from the float64 restatement, largest {diff.max()}')
    assert diff.max() <= 1


def test_shade_on_rendered_bodies_front_and_side(body):
    report = _mod('report')
    verts, cam, p2f = body['verts'], body['cam'], body['p2f']
    normals, rgb, depth, nmap, status = _shade_body(body, verts, p2f)
    covered = (p2f >= 0).cpu().numpy()
    print(f'front: covered pixels per pose {covered.reshape(3, -1).sum(1).tolist()}')
    assert status == 0 and (covered.reshape(3, -1).sum(1) > 1000).all()
    assert ((depth >= 0) == covered).all() and (rgb.any(-1) == covered).all() and ((nmap != 0).any(-1) == covered).all()
    assert np.abs(np.linalg.norm(nmap[covered].astype(F64), axis=-1) - 1).max() <= 1e-5
    _against_restatement('body front', body, verts, normals, p2f, rgb, depth, nmap)
    # the side view: the same camera, the body turned about its centroid
    turned = report.side_view(verts, cam).contiguous()
    body['eng'].silhouette_forward(turned, cam)
    p2f_s = body['eng'].silhouette_pix_to_face()
    normals_s, rgb_s, depth_s, nmap_s, status_s = _shade_body(body, turned, p2f_s)
    covered_s = (p2f_s >= 0).cpu().numpy()
    print(f'side: covered pixels per pose {covered_s.reshape(3, -1).sum(1).tolist()}')
    assert status_s == 0 and (covered_s.reshape(3, -1).sum(1) > 0).all() and (covered_s != covered).reshape(3, -1).any(1).all()
    assert ((depth_s >= 0) == covered_s).all() and (rgb_s.any(-1) == covered_s).all()
    assert np.abs(np.linalg.norm(nmap_s[covered_s].astype(F64), axis=-1) - 1).max() <= 1e-5
    _against_restatement('body side', body, turned, normals_s, p2f_s, rgb_s, depth_s, nmap_s)
    # its depths stay within the body's extent of the front view's centroid depth
    view = body['v_np'].astype(F64) * [-2.0, -2.0, 2.0] + cam.cpu().numpy().astype(F64)[:, None]
    centre = view.mean(1)
    extent = np.linalg.norm(view - centre[:, None], axis=-1).max(1)
    for b in range(3):
        d = depth_s[b][covered_s[b]]
        print(f'side pose {b}: depth {d.min():.3f} .. {d.max():.3f}, centroid {centre[b, 2]:.3f}, extent {extent[b]:.3f}')
        assert centre[b, 2] - extent[b] - 1e-3 <= d.min() and d.max() <= centre[b, 2] + extent[b] + 1e-3


def test_mesh_renderer_shaded_at_64(body, smpl_hip):
    report = _mod('report')
    r = _mod('mesh_renderer').Mesh_Renderer(64, smpl=smpl_hip)
    smpl_verts = body['verts'] * body['verts'].new_tensor([-2.0, -2.0, 2.0])
    batch = {'cam': body['cam']}
    front = r.shaded(batch, smpl_verts)
    assert front.shape == (3, 64, 64, 3) and front.dtype == torch.uint8
    p2f = r._engine(3).silhouette_pix_to_face()
    assert tuple(p2f.shape) == (3, 64, 64)
    covered = (p2f >= 0).cpu().numpy()
    assert (front.cpu().numpy().any(-1) == covered).all() and (covered.reshape(3, -1).sum(1) > 80).all()
    a = (body['v_np'], body['normals'].cpu().numpy(), body['faces'], body['cam'].cpu().numpy(), p2f.cpu().numpy())
    diff = np.abs(front.cpu().numpy().astype(np.int64) - msc.shade_ref(*a, F64)['rgb'].astype(np.int64))
    print(f'Mesh_Renderer(64).shaded: {(diff != 0).sum()} of {diff.size} bytes differ from the float64 restatement, largest {diff.max()}')
    assert diff.max() <= 1
    image = T(msc.background_image(3, 64)).to(DEV)
    over = r.shaded(batch, smpl_verts, image=image).cpu().numpy()
    want_bg = np.floor(np.clip(image.cpu().numpy().transpose(0, 2, 3, 1), 0, 1) * F32(255) + F32(0.5)).astype(np.uint8)
    assert np.array_equal(over[~covered], want_bg[~covered]) and np.array_equal(over[covered], front.cpu().numpy()[covered])
    side = r.shaded(batch, smpl_verts, side=True).cpu().numpy()
    covered_s = (r._engine(3).silhouette_pix_to_face() >= 0).cpu().numpy()
    grey = int(np.floor(F32(report.SIDE_GREY) * F32(255) + F32(0.5)))
    assert side.shape == (3, 64, 64, 3) and (side[~covered_s] == grey).all() and covered_s.any() and (covered_s != covered).any()
    with pytest.raises(NotImplementedError):
        _mod('mesh_renderer').Mesh_Renderer(100)


# ---- 4. the driver ----
DRIVER_FLAGS = ['--batch_size', '8', '--synthetic_batches', '1', '--inner_iters', '3', '--camera_iters', '5', '--silhouette', '--reprojection',
                '--synthetic', '--device', DEV]


def _driver(flags):
    argsmod = _mod('args')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(flags + ['--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent'])
    try:
        torch.manual_seed(0)
        return _mod('optimize').optimize_pose_refiner(log=lambda r: None)
    finally:
        argsmod._LazyArgs._ns = saved


def test_driver_fit_report_mesh(tmp_path):
    with_dir, plain_dir = str(tmp_path / 'mesh'), str(tmp_path / 'plain')
    res = _driver(DRIVER_FLAGS + ['--fit_report', with_dir, '--fit_report_images', '3', '--fit_report_mesh'])
    plain = _driver(DRIVER_FLAGS + ['--fit_report', plain_dir, '--fit_report_images', '3'])
    overlays = sorted(f'b0000_p{p:05d}_{w}.png' for p in range(3) for w in ('before', 'after'))
    meshes = sorted(f'b0000_p{p:05d}_{w}_mesh.png' for p in range(3) for w in ('before', 'after'))
    assert sorted(os.listdir(plain_dir)) == overlays and sorted(os.listdir(with_dir)) == sorted(overlays + meshes)
    for name in overlays:                # today's pictures: the same bytes
        assert open(os.path.join(with_dir, name), 'rb').read() == open(os.path.join(plain_dir, name), 'rb').read(), name
    grey = int(np.floor(F32(_mod('report').SIDE_GREY) * F32(255) + F32(0.5)))
    for name in meshes:
        rgb, _ = frc.read_png(os.path.join(with_dir, name))
        assert rgb.shape == (224, 448, 3)
        left, right = rgb[:, :224], rgb[:, 224:]
        assert left.min() != left.max() and right.min() != right.max()              # non-constant in both halves
        assert (left[0, 0] == 0).all() and (right[0, 0] == grey).all()              # the body over black, its side view over grey
        assert 1000 < left.any(-1).sum() < 224 * 224 // 2 and 0 < (right != grey).any(-1).sum() < 224 * 224 // 2
    # the refinement itself is the same to the bit
    for k in ('x6d', 'betas', 'cam', 'J_regressor'):
        assert torch.equal(res[k], plain[k]), k
    assert res['history'][0]['silhouette_iou_after'] == plain['history'][0]['silhouette_iou_after']


def test_two_ranks_write_their_own_shards_mesh_pictures(tmp_path):
    """the driver in rank processes of their own (tests/dp_worker.py): two ranks over gloo sharing cuda:0"""
    tmp = str(tmp_path)
    worker = os.path.join(ROOT, 'tests', 'dp_worker.py')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1', '--master-port',
           '29571', worker, os.path.join(tmp, 'w2')] + DRIVER_FLAGS + ['--fit_report_images', '1', '--fit_report', os.path.join(tmp, 'png2'),
                                                                       '--fit_report_mesh', '--dist_backend', 'gloo', '--single_device']
    p = subprocess.Popen(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        text, rc = p.communicate(timeout=600)[0], p.returncode
    except subprocess.TimeoutExpired:
        p.kill()
        text, rc = p.communicate()[0], -999
    assert rc == 0, f'two ranks failed (rc {rc}):\n{text[-3000:]}'
    shards = [(int(r['lo']), int(r['hi'])) for r in (dict(np.load(os.path.join(tmp, f'w2.rank{k}.npz'))) for k in (0, 1))]
    assert shards == [(0, 4), (4, 8)]
    # every rank writes the first pose of ITS shard, named by the global pose
    assert sorted(os.listdir(os.path.join(tmp, 'png2'))) == sorted(f'b0000_p{p:05d}_{w}{m}.png' for p in (0, 4) for w in ('before', 'after')
                                                                   for m in ('', '_mesh'))
    pictures = {}
    for p_ in (0, 4):
        for w in ('before', 'after'):
            rgb, _ = frc.read_png(os.path.join(tmp, 'png2', f'b0000_p{p_:05d}_{w}_mesh.png'))
            assert rgb.shape == (224, 448, 3) and rgb[:, :224].any() and rgb[:, 224:].min() != rgb[:, 224:].max()
            pictures[p_, w] = rgb
    assert not np.array_equal(pictures[0, 'before'], pictures[4, 'before'])          # two different poses
