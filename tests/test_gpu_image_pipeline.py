"""The device image pipeline through the C ABI (pytest -m gpu): jrr_image_crop against the reference's own crops
(tests/golden/g9_find_crop.npz) and against the host find_crop on 1000-px frames, its launch variants bit for bit, the status word,
jrr_mask_prepare, and the driver fitting the dataset's masks (`--image_masks`).

Bound of a crop: 3 x ref_f64_err of the frame class + 1e-7 (tests/test_image_pipeline.py; the fixture's two scalars)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import PKG_NAME, load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_cases as ic  # noqa: E402

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _whole(frames):
    return torch.tensor([[0, 0, f.shape[0], f.shape[1]] for f in frames])


def _crop(frames, bboxes, sizes, rois=None, normalize=None):
    """jrr_image_crop on a list of uint8 frames; returns (crops, status word)"""
    d = _mod('data')
    pix, desc = d.pack_frames(frames, _whole(frames) if rois is None else rois)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    outs = d.image_crop(pix.to(DEV), desc.to(DEV), torch.as_tensor(bboxes, dtype=torch.float32).to(DEV).contiguous(), sizes, normalize, status)
    return [o.cpu() for o in outs], int(status.item())


def test_image_crop_small_cases_against_the_reference():
    g = load_golden('g9_find_crop.npz')
    bound = 3 * float(g['ref_f64_err_small']) + 1e-7
    frames = ic.small_frames()
    for name, fnames, bboxes, n in ic.SMALL_CASES:
        (crop,), status = _crop([frames[f] for f in fnames], bboxes, (n,))
        ref = g[f'{name}__crop']
        err = np.abs(crop.numpy() - ref).max()
        print(f'{name}: |crop - reference| = {err:.3e} (bound {bound:.3e})')
        assert status == 0, name
        assert crop.shape == ref.shape and err <= bound, (name, err, bound)
        if name in ic.ALL_ZERO_CASES:
            assert not crop.numpy().any(), name


@pytest.fixture(scope='module')
def large():
    """the 37 x 2 large cases: frames, bboxes and the host find_crop at 224 and 256"""
    d = _mod('data')
    big = ic.large_frames()
    bbs = T(ic.large_bboxes())
    frames = [big['noise']] * len(bbs) + [big['smooth']] * len(bbs)
    bboxes = torch.cat([bbs, bbs])
    k = T(ic.small_intrinsics(len(bboxes)))
    host = {}
    for n in (224, 256):
        host[n] = torch.cat([d.find_crop(T(f).permute(2, 0, 1)[:, :1000, :1000].float() / 255.0, bboxes[i:i + 1], k[i:i + 1], img_size=n)[0]
                             for i, f in enumerate(frames)])
    return frames, bboxes, k, host


def test_image_crop_large_frames_against_host(large):
    d = _mod('data')
    frames, bboxes, k, host = large
    bound = 3 * float(load_golden('g9_find_crop.npz')['ref_f64_err_1000']) + 1e-7
    rs = np.random.RandomState(3)
    masks = [rs.randint(0, 256, size=(224, 224)).astype(np.uint8) for _ in frames]
    out = d.crop_batch(frames, masks, bboxes, k, DEV)                       # 1002-row frames: cut to 1000 x 1000 inside
    assert out['spin_image'].shape == (74, 3, 224, 224) and out['image'].shape == (74, 3, 256, 256)
    assert out['bytes_uploaded'] < 0.6 * 74 * 3e6                            # the blocks, not the frames
    for key, n in (('spin_image', 224), ('image', 256)):
        err = (out[key].cpu() - host[n]).abs().amax((1, 2, 3))
        print(f'{key}: largest |device - host| = {err.max().item():.3e} (bound {bound:.3e}); samples that differ at all: {int((err > 0).sum())}')
        assert err.max().item() <= bound
        assert not out[key][35].any() and not out[key][36].any()            # wholly outside, zero size
    geo = d.find_crop(torch.zeros(74, 3, 8, 8), bboxes, k, img_size=256)
    np.testing.assert_allclose(out['intrinsics'].cpu().numpy(), geo[4].numpy(), rtol=1e-6, equal_nan=True)
    for key, ref in (('min_x', geo[1]), ('min_y', geo[2]), ('scale', geo[3])):
        np.testing.assert_allclose(out[key].cpu().numpy(), ref.numpy(), rtol=1e-6)
    want = T(np.stack(masks)).float()[:, None] / 255.0
    assert out['valid'].cpu().tolist() == [bool(m[0, 0]) for m in masks]
    want[:, :, :2, :2] = 0
    assert torch.equal(out['mask_rcnn'].cpu(), want)


def test_image_crop_launch_variants_bit_for_bit(large):
    d = _mod('data')
    frames, bboxes, k, _ = large
    frames = [f[:1000, :1000] for f in frames[30:44]]                        # seven bboxes on each of the two frames
    bboxes = bboxes[30:44]
    both, status = _crop(frames, bboxes, (224, 256))
    assert status == 0
    for i, n in enumerate((224, 256)):                                      # two sizes from one launch = two launches
        (single,), status = _crop(frames, bboxes, (n,))
        assert status == 0 and torch.equal(single, both[i]), n
    rois = d.crop_roi(bboxes, 1000, 1000)
    assert (rois[:, 2] * rois[:, 3]).sum().item() < 0.6 * len(frames) * 1e6
    blocks, status = _crop(frames, bboxes, (224, 256), rois=rois)            # blocks = whole frames
    assert status == 0 and torch.equal(blocks[0], both[0]) and torch.equal(blocks[1], both[1])
    # a block one row short: an argument check (the kernel reads nothing outside what it was given), reported through the status word
    short = rois.clone()
    b = int(torch.nonzero(short[:, 2] > 8)[0])
    short[b, 2] -= 1
    _, status = _crop(frames, bboxes, (224, 256), rois=short)
    assert status & 1
    masks = [np.zeros((224, 224), np.uint8)] * len(frames)
    with pytest.raises(_mod('_lib').JrrError, match='region of interest'):
        d.crop_batch(frames, masks, bboxes, k[30:44], DEV, rois=short)
    # a descriptor that points past the buffer is refused by the kernel before it reads
    pix, desc = d.pack_frames(frames[:1], _whole(frames[:1]))
    desc[0, 0] = pix.numel()
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = d.image_crop(pix.to(DEV), desc.to(DEV), bboxes[:1].to(DEV).contiguous(), (32,), None, status)
    assert int(status.item()) & 2 and not out[0].any()


def test_image_crop_normalize(large):
    d = _mod('data')
    frames, bboxes, _, _ = large
    frames, bboxes = [f[:1000, :1000] for f in frames[:6]], bboxes[:6]
    plain, _ = _crop(frames, bboxes, (224, 256))
    normed, status = _crop(frames, bboxes, (224, 256), normalize=d.SPIN_NORMALIZE)
    mean, std = (torch.tensor(v).view(1, 3, 1, 1) for v in d.SPIN_NORMALIZE)
    np.testing.assert_allclose(normed[0].numpy(), ((plain[0] - mean) / std).numpy(), rtol=2.4e-7, atol=1e-7)
    assert status == 0 and torch.equal(normed[1], plain[1])                  # the 256 crop is not normalised (scripts/optimize.py:164)


def test_mask_prepare_exact():
    d = _mod('data')
    rs = np.random.RandomState(8)
    for shape in ((8, 224, 224), (3, 5, 7), (1, 2, 2)):
        m = rs.randint(0, 256, size=shape).astype(np.uint8)
        m[0, 0, 0] = 0
        got, valid = d.mask_prepare(T(m).to(DEV))
        want = T(m).float().unsqueeze(1) / 255.0
        want_valid = want[:, 0, 0, 0] != 0
        want[:, :, :2, :2] = 0
        assert torch.equal(got.cpu(), want) and torch.equal(valid.cpu(), want_valid), shape


def test_driver_fits_the_datasets_masks(tmp_path):
    """optimize_pose_refiner in-process on a dataset of 8 samples with .npy frames and 224 x 224 masks: the silhouette term of
    iteration 0 is 100 * mean((alpha - mask)^2) against the PREPARED dataset masks"""
    sm, argsmod, opt, em, d = _mod('smpl_model'), _mod('args'), _mod('optimize'), _mod('engine'), _mod('data')
    B = 8
    smpl = _mod('smpl').SMPL('SPIN/data/smpl', batch_size=1, allow_synthetic=True)
    J = sm.default_h36m_regressor()
    batch = sm.synthetic_batch(smpl.model_np, J, B, seed=17)
    x6, betas, cam = T(batch['pose6d']).contiguous(), T(batch['betas']).contiguous(), T(batch['cam']).contiguous()
    eng = em.RefineEngine(smpl.to(DEV).device_model, B, flags=em.FLAG_SILHOUETTE | em.FLAG_KEEP_VERTS)
    eng.set_j_regressor(T(J).to(DEV))
    _, verts = eng.find_joints_forward(betas.to(DEV), x6d=x6.to(DEV), return_verts=True)
    moved = (cam + torch.tensor([0.15, -0.1, 1.0])).to(DEV).contiguous()
    masks = ((eng.silhouette_forward(verts, moved) > 0).cpu().numpy() * 255).astype(np.uint8)
    assert masks.shape == (B, 224, 224) and 1000 < int((masks[0] > 0).sum()) < 40000
    masks[3, 0, 0] = 255                                                   # one sample with valid == True
    loc = tmp_path / 'precomputed_val'
    loc.mkdir()
    bbs = T(ic.large_bboxes()[:B])
    files = dict(bboxes=bbs, betas=betas, estimated_translation=cam, gt_j2d=torch.rand(B, 17, 2) * 1000, gt_j3d=T(batch['gt_j3d']),
                 intrinsics=T(ic.small_intrinsics(B)), orient=x6[:, :1], pose=x6[:, 1:])
    for k, v in files.items():
        torch.save(v.clone(), str(loc / f'{k}.pt'))
    for i in range(B):
        np.save(loc / f'frame_{i:06d}.npy', ic.noise_frame(120, 160, 100 + i))
        np.save(loc / f'mask_{i:06d}.npy', masks[i])
    prepared, valid = d.mask_prepare(T(masks).to(DEV))
    alpha = eng.silhouette_forward(verts, cam.to(DEV))
    want = 100 * ((alpha - prepared[:, 0]) ** 2).mean().item()
    flags = ['--batch_size', str(B), '--inner_iters', '2', '--device', DEV, '--data_root', str(tmp_path), '--silhouette']
    recs = {}
    for name, extra in (('dataset', ['--image_masks']), ('synthetic', [])):
        argsmod._LazyArgs._ns = argsmod.get_args(flags + extra)
        recs[name] = opt.optimize_pose_refiner(log=lambda r: None)['history'][0]
    rec = recs['dataset']
    got = rec['loss_history'][0][1]
    print(f'silhouette term at iteration 0: driver {got:.6f}, 100 * mean((alpha - mask)^2) {want:.6f}, synthetic masks {recs["synthetic"]["loss_history"][0][1]:.6f}')
    assert rec['masks'] == 'dataset' and rec['data'] == 'dataset' and rec['masks_invalid'] == B - 1 == int((~valid).sum())
    np.testing.assert_allclose(got, want, rtol=2e-4)
    assert recs['synthetic']['masks'] == 'synthetic' and recs['synthetic']['masks_invalid'] is None
    assert abs(recs['synthetic']['loss_history'][0][1] - want) > 1e-2 * want
    # a mask of another size is an error that names the sample
    np.save(loc / 'mask_000005.npy', masks[5][:200, :200].copy())
    argsmod._LazyArgs._ns = argsmod.get_args(flags + ['--image_masks'])
    with pytest.raises(ValueError, match='sample 5'):
        opt.optimize_pose_refiner(log=lambda r: None)
