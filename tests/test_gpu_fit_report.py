"""The fit report on the GPU (pytest -m gpu): jrr_silhouette_compare and jrr_fit_overlay against the host restatement of
/root/reference/scripts/optimize.py:28-74 (tests/fit_report_cases.py) -- integer counts and bytes, so every comparison is exact --,
`--fit_report` through the driver (:204-218 before the loop, :268-274 after it), and two gloo ranks against one.

Shapes: 4 x 4 (fewer pixels than a wave), 36 x 20 (h * w no multiple of 256), 32 x 32, 224² (the loop's size) and 256² (the largest:
64 workgroups per pose in both kernels).
"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fit_report_cases as frc
from conftest import PKG_NAME, ROOT

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


@pytest.fixture(scope='module')
def smpl_hip(smpl_model_np):
    return _mod('smpl').SMPL(model=smpl_model_np).to(DEV)


# ---- 1. compare, exact ----
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('h,w', [(4, 4), (36, 20), (32, 32), (224, 224), (256, 256)])
def test_compare_counts_equal_the_restatement(h, w, B):
    report = _mod('report')
    alpha, mask = frc.compare_case(B, h, w)
    want = frc.compare_ref(alpha, mask)
    assert want[0, 2] > 0 and want[0, 3] > 0 and want[0, 0] < want[0, 1]
    ad, md = T(alpha).to(DEV), T(mask).to(DEV)
    got = report.silhouette_compare(ad, md)
    assert got.dtype == torch.int32 and got.shape == (B, 4)
    print(f'compare {h}x{w} B={B}: counts {got.cpu().tolist()} restatement {want.tolist()}')
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(report.silhouette_compare(ad[:, None], md[:, None]).cpu().numpy(), want)        # (B,1,h,w) as well
    iou = report.silhouette_iou(ad, md)
    assert iou.dtype == torch.float64 and np.array_equal(iou.cpu().numpy(), frc.iou_ref(alpha, mask))
    if B == 3:
        assert want[1].tolist() == [0, 0, 0, 0] and want[2].tolist() == [h * w] * 4
        assert iou.cpu().tolist()[1:] == [1.0, 1.0]                  # both empty: they agree; both full
    # other thresholds: strict on both sides
    got2 = report.silhouette_compare(ad, md, thr_render=0.25, thr_mask=float(np.float32(100) / np.float32(255)))
    assert np.array_equal(got2.cpu().numpy(), frc.compare_ref(alpha, mask, 0.25, float(np.float32(100) / np.float32(255))))


def test_compare_refuses_a_pixel_count_that_is_no_multiple_of_four():
    lib_mod = _mod('_lib')
    lib = lib_mod.load()
    a = torch.ones(2, 5, 3, device=DEV)
    counts = torch.full((2, 4), -7, dtype=torch.int32, device=DEV)
    rc = lib.jrr_silhouette_compare(lib_mod.ptr(a), lib_mod.ptr(a), 2, 5, 3, 0.5, 0.8, lib_mod.ptr(counts), lib_mod.stream_ptr(a.device))
    torch.cuda.synchronize()
    assert rc == -1 and b'multiple of 4' in lib.jrr_last_error()
    assert (counts == -7).all().item()                               # nothing written, not even the zeroing
    with pytest.raises(lib_mod.JrrError):
        _mod('report').silhouette_compare(a, a)


# ---- 2. compare on rendered silhouettes ----
def test_compare_on_rendered_silhouettes(smpl_hip, smpl_model_np, j_h36m_np):
    eng_mod, report = _mod('engine'), _mod('report')
    B = 3
    batch = _mod('smpl_model').synthetic_batch(smpl_model_np, j_h36m_np, B, seed=31)
    eng = eng_mod.RefineEngine(smpl_hip.device_model, B, flags=eng_mod.FLAG_SILHOUETTE | eng_mod.FLAG_KEEP_VERTS)
    eng.set_j_regressor(T(j_h36m_np))
    xd, bd, cd = (T(batch[k]).to(DEV).contiguous() for k in ('pose6d', 'betas', 'cam'))
    _, verts = eng.find_joints_forward(bd, x6d=xd, return_verts=True)
    alpha = eng.silhouette_forward(verts, cd)
    assert alpha.shape == (B, 224, 224)
    mask = (torch.roll(alpha, shifts=(9, -6), dims=(1, 2)) > 0).float().contiguous()
    got = report.silhouette_compare(alpha, mask).cpu().numpy()
    want = frc.compare_ref(alpha.cpu().numpy(), mask.cpu().numpy())
    print(f'rendered: counts {got.tolist()}')
    assert np.array_equal(got, want)
    assert (want[:, 0] > 1000).all() and (want[:, 0] < want[:, 1]).all()          # a body, and the shift shows
    soft = ((alpha > 0) & (alpha < 1)).sum().item()
    assert soft > 100                                                             # the soft rim crosses the threshold somewhere


# ---- 3. overlay, exact ----
VARIANTS = {'bare': (0, False, False, 2.0), 'image_one_set': (1, True, False, 1.25), 'normalised_three_sets': (3, True, True, 2.5),
            'three_sets_no_image': (3, False, False, 1.0)}


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('S', [4, 32, 224])
def test_overlay_bytes_equal_the_restatement(S, B, variant):
    report, data = _mod('report'), _mod('data')
    n_sets, with_image, with_norm, radius = VARIANTS[variant]
    alpha, mask, image, sets = frc.overlay_case(B, S, n_sets, with_image, radius)
    normalize = data.SPIN_NORMALIZE if with_norm else None
    if with_norm:            # the picture arrives normalised, as the SPIN network takes it
        mean, std = (np.asarray(v, dtype=np.float32).reshape(1, 3, 1, 1) for v in normalize)
        image = ((image - mean) / std).astype(np.float32)
    want = frc.overlay_ref(alpha, mask, image, normalize, sets, radius)
    # 64 guard bytes on either side of the output
    n = B * S * S * 3
    buf = torch.full((n + 128,), 0xA5, dtype=torch.uint8, device=DEV)
    out = buf[64:64 + n].view(B, S, S, 3)
    got = report.fit_overlay(T(alpha).to(DEV), T(mask).to(DEV), image=T(image).to(DEV) if with_image else None, normalize=normalize,
                             joints2d=[T(s).to(DEV) for s in sets], radius=radius, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.dtype == torch.uint8 and got.shape == (B, S, S, 3)
    host = buf.cpu().numpy()
    assert (host[:64] == 0xA5).all() and (host[-64:] == 0xA5).all()
    diff = int((host[64:-64].reshape(B, S, S, 3) != want).sum())
    print(f'overlay S={S} B={B} {variant}: {diff} of {n} bytes differ')
    assert np.array_equal(host[64:-64].reshape(B, S, S, 3), want)
    if n_sets and S >= 32:   # the planted joints drew: both corners, the rim pixel; the last set's colour on top
        top = np.asarray(frc.SET_COLOURS[n_sets - 1], dtype=np.uint8)
        frac = radius - np.floor(radius)
        assert (want[:, 0, 0] == top).all() and (want[:, S - 1, S - 1] == top).all()
        assert (want[:, S // 2, int(S // 2 - frac + radius)] == top).all()
    # an allocation of its own, (B,1,S,S) inputs
    again = report.fit_overlay(T(alpha).to(DEV)[:, None], T(mask).to(DEV)[:, None], image=T(image).to(DEV) if with_image else None,
                               normalize=normalize, joints2d=[T(s).to(DEV) for s in sets], radius=radius)
    assert np.array_equal(again.cpu().numpy(), want)


# ---- 4. the driver ----
DRIVER_FLAGS = ['--batch_size', '8', '--synthetic_batches', '1', '--inner_iters', '3', '--camera_iters', '5', '--silhouette', '--reprojection',
                '--synthetic', '--device', DEV]


def _driver(flags, monkeypatch=None, seen=None):
    argsmod = _mod('args')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(flags + ['--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent'])
    opt = _mod('optimize')
    if seen is not None:
        mask_fn = opt._synthetic_mask

        def mask_spy(*a):
            seen['mask'] = mask_fn(*a)
            return seen['mask']
        monkeypatch.setattr(opt, '_synthetic_mask', mask_spy)
    try:
        torch.manual_seed(0)
        return opt.optimize_pose_refiner(log=lambda r: None)
    finally:
        argsmod._LazyArgs._ns = saved


def test_driver_fit_report(tmp_path, monkeypatch, smpl_hip):
    eng_mod, report = _mod('engine'), _mod('report')
    out_dir = str(tmp_path / 'fit')
    seen = {}
    res = _driver(DRIVER_FLAGS + ['--fit_report', out_dir, '--fit_report_images', '3'], monkeypatch, seen)
    monkeypatch.undo()
    plain = _driver(DRIVER_FLAGS)
    rec = res['history'][0]
    print({k: rec[k] for k in ('silhouette_iou_before', 'silhouette_iou_after', 'j2d_error_px_before', 'j2d_error_px_after')})
    for k in ('silhouette_iou_before', 'silhouette_iou_after'):
        assert isinstance(rec[k], float) and np.isfinite(rec[k]) and 0.0 <= rec[k] <= 1.0, (k, rec[k])
    for k in ('j2d_error_px_before', 'j2d_error_px_after'):
        assert isinstance(rec[k], float) and np.isfinite(rec[k]) and rec[k] >= 0.0, (k, rec[k])
    assert not any(k.startswith(('silhouette_iou', 'j2d_error')) for k in plain['history'][0]) and 'fit_report' not in plain
    # exactly 3 x 2 pictures of 224 x 224
    names = sorted(os.listdir(out_dir))
    assert names == sorted(f'b0000_p{p:05d}_{w}.png' for p in range(3) for w in ('before', 'after'))
    for name in names:
        rgb, _ = frc.read_png(os.path.join(out_dir, name))
        assert rgb.shape == (224, 224, 3) and rgb.any()
        green = (rgb == np.array([0, 255, 0], dtype=np.uint8)).all(-1).sum()
        assert green > 0                                              # target joints (discs) in every picture
    # the refinement itself is the same to the bit
    for k in ('x6d', 'betas', 'cam', 'J_regressor'):
        assert torch.equal(res[k], plain[k]), k
    # the IoU of the record, recomputed from the returned final state and the same mask
    eng = eng_mod.RefineEngine(smpl_hip.device_model, 8, flags=eng_mod.FLAG_SILHOUETTE | eng_mod.FLAG_KEEP_VERTS)
    eng.set_j_regressor(res['J_regressor'])
    _, verts = eng.find_joints_forward(res['betas'], x6d=res['x6d'], return_verts=True)
    iou = report.silhouette_iou(eng.silhouette_forward(verts, res['cam']), seen['mask'])
    print(f"iou after: record {rec['silhouette_iou_after']!r} recomputed {iou.mean().item()!r}")
    assert abs(rec['silhouette_iou_after'] - iou.mean().item()) <= 1e-12
    assert res['fit_report']['shard'] == (0, 8)
    assert np.array_equal(res['fit_report']['iou_after'], iou.cpu().numpy())
    assert abs(rec['silhouette_iou_before'] - res['fit_report']['iou_before'].mean()) <= 1e-12


# ---- 5. two gloo ranks on one GPU ----
@pytest.fixture(scope='module')
def rank_runs(tmp_path_factory):
    """the driver in rank processes of their own (tests/dp_worker.py): one rank, and two ranks over gloo sharing cuda:0"""
    tmp = str(tmp_path_factory.mktemp('fit_dp'))
    worker = os.path.join(ROOT, 'tests', 'dp_worker.py')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    flags = DRIVER_FLAGS + ['--fit_report_images', '1']
    cmds = {
        'w1': [sys.executable, worker, os.path.join(tmp, 'w1')] + flags + ['--fit_report', os.path.join(tmp, 'png1')],
        'w2': [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
               '--master-port', '29561', worker, os.path.join(tmp, 'w2')] + flags
              + ['--fit_report', os.path.join(tmp, 'png2'), '--dist_backend', 'gloo', '--single_device'],
    }
    procs = {k: subprocess.Popen(c, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for k, c in cmds.items()}
    outs = {}
    for k, p in procs.items():
        try:
            outs[k] = (p.communicate(timeout=600)[0], p.returncode)
        except subprocess.TimeoutExpired:
            p.kill()
            outs[k] = (p.communicate()[0], -999)
    for k, (text, rc) in outs.items():
        assert rc == 0, f'{k} failed (rc {rc}):\n{text[-3000:]}'
    return tmp


def test_two_ranks_report_what_one_rank_reports(rank_runs):
    load = lambda name: dict(np.load(os.path.join(rank_runs, name)))
    one, two = load('w1.rank0.npz'), [load('w2.rank0.npz'), load('w2.rank1.npz')]
    assert [(int(r['lo']), int(r['hi'])) for r in two] == [(0, 4), (4, 8)]
    h1 = json.loads(str(one['history']))[0]
    for r in two:
        h2 = json.loads(str(r['history']))[0]
        print({k: (h1[k], h2[k]) for k in ('silhouette_iou_before', 'silhouette_iou_after', 'j2d_error_px_before', 'j2d_error_px_after')})
        # integer ratios summed in float64
        assert abs(h2['silhouette_iou_before'] - h1['silhouette_iou_before']) <= 1e-12
        assert abs(h2['silhouette_iou_after'] - h1['silhouette_iou_after']) <= 1e-12
        # fp32 means whose summation order differs between the shard sizes
        assert abs(h2['j2d_error_px_before'] - h1['j2d_error_px_before']) <= 1e-5 * abs(h1['j2d_error_px_before'])
        assert abs(h2['j2d_error_px_after'] - h1['j2d_error_px_after']) <= 1e-5 * abs(h1['j2d_error_px_after'])
    # every rank writes the first pose of ITS shard, named by the global pose
    assert sorted(os.listdir(os.path.join(rank_runs, 'png1'))) == ['b0000_p00000_after.png', 'b0000_p00000_before.png']
    assert sorted(os.listdir(os.path.join(rank_runs, 'png2'))) == ['b0000_p00000_after.png', 'b0000_p00000_before.png',
                                                                  'b0000_p00004_after.png', 'b0000_p00004_before.png']
    for name in os.listdir(os.path.join(rank_runs, 'png2')):
        assert frc.read_png(os.path.join(rank_runs, 'png2', name))[0].shape == (224, 224, 3)
