"""CPU checks of the dataset image pipeline (data.py): the host find_crop against the reference's own output
(tests/golden/g9_find_crop.npz, written by tests/golden/make_golden_images.py), the image-valued keys of data_set, the region of
interest the device route uploads, and the driver flag.

Bound of a crop against the reference: 3 x ref_f64_err of the frame class + 1e-7 (pixel values are in [0, 1]) -- once for the
reference's own distance from the float64 evaluation of its formulas, twice for an implementation whose position arithmetic rounds
in another order.  ref_f64_err is stored in the fixture by the generator (8.7e-6 small frames, 1.6e-4 1000-px frames); it does not
depend on the code under test."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import PKG_NAME, load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_cases as ic  # noqa: E402

T = torch.from_numpy


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def to_image(frame):
    return T(frame).permute(2, 0, 1)[:, :1000, :1000].float() / 255.0


def test_linspace_formula_is_torchs_up_to_its_vector_width():
    """data.linspace_pm1 (repeated by csrc/image.hip lin_pm1) is torch.linspace's scalar formula; torch.linspace itself may differ in
    the last bit (it fills SIMD vectors from one base value): at most one unit in the last place of 1"""
    d = _mod('data')
    for n in range(4, 257, 4):
        mine, ref = d.linspace_pm1(n), torch.linspace(-1.0, 1.0, n)
        assert mine.dtype == torch.float32 and mine[0] == -1 and mine[-1] == 1
        assert (mine - ref).abs().max().item() <= 2.0 ** -23, n


def test_host_find_crop_against_the_reference():
    d = _mod('data')
    g = load_golden('g9_find_crop.npz')
    bound = 3 * float(g['ref_f64_err_small']) + 1e-7
    assert 1e-6 < float(g['ref_f64_err_small']) < 5e-5 and 2e-5 < float(g['ref_f64_err_1000']) < 1e-3      # fp32 position error, not a defect
    frames = ic.small_frames()
    worst = 0.0
    for name, fnames, bboxes, n in ic.SMALL_CASES:
        image = torch.stack([to_image(frames[f]) for f in fnames])
        bb, k = torch.tensor(bboxes), T(ic.small_intrinsics(len(fnames)))
        crop, min_x, min_y, scale, k2 = d.find_crop(image if len(fnames) > 1 else image[0], bb, k, img_size=n)
        ref = g[f'{name}__crop']
        assert crop.shape == ref.shape == (len(fnames), 3, n, n)
        err = np.abs(crop.numpy() - ref).max()                      # every pixel of every case
        worst = max(worst, err)
        print(f'{name}: |crop - reference| = {err:.3e} (bound {bound:.3e})')
        assert err <= bound, (name, err, bound)
        if name in ic.ALL_ZERO_CASES:
            assert not ref.any() and not crop.numpy().any(), name
        np.testing.assert_allclose(min_x.numpy(), g[f'{name}__min_x'], rtol=1e-6)
        np.testing.assert_allclose(min_y.numpy(), g[f'{name}__min_y'], rtol=1e-6)
        np.testing.assert_allclose(scale.numpy(), g[f'{name}__scale'], rtol=1e-6)
        if name in ic.ZERO_SIZE_CASES:
            assert not np.isfinite(g[f'{name}__intrinsics']).all()
            np.testing.assert_allclose(k2.numpy(), g[f'{name}__intrinsics'], rtol=1e-6, equal_nan=True)
        else:
            np.testing.assert_allclose(k2.numpy(), g[f'{name}__intrinsics'], rtol=1e-6)
        assert torch.equal(torch.stack(d.crop_params(bb)), torch.stack([min_x, min_y, scale]))         # crop_params is the same geometry
    assert worst > 0          # the comparison saw real pixels


def test_intrinsics_functions_have_the_reference_signatures():
    d = _mod('data')
    k = T(ic.small_intrinsics(2))
    c = d.crop_intrinsics(k, torch.tensor([600., 400.]), torch.tensor([600., 400.]), torch.tensor([400., 300.]), torch.tensor([450., 350.]))
    np.testing.assert_allclose(c[:, 0, 2].numpy(), k[:, 0, 2].numpy() + np.array([299.5, 199.5]) - np.array([450., 350.]), rtol=1e-6)
    np.testing.assert_allclose(c[:, 1, 2].numpy(), k[:, 1, 2].numpy() + np.array([299.5, 199.5]) - np.array([400., 300.]), rtol=1e-6)
    r = d.resize_intrinsics(k, 1000.0, 1000.0, 0.5)
    np.testing.assert_allclose(r[:, 0, 0].numpy(), 0.5 * k[:, 0, 0].numpy(), rtol=1e-6)
    np.testing.assert_allclose(r[:, 0, 2].numpy(), 249.5 + 0.5 * (k[:, 0, 2].numpy() - 499.5), rtol=1e-6)
    assert torch.equal(r[:, 2], k[:, 2]) and torch.equal(c[:, :, :2], k[:, :, :2])


def _write_split(tmp_path, n, bboxes=None, seed=0):
    loc = tmp_path / 'precomputed_val'
    loc.mkdir()
    g = torch.Generator().manual_seed(seed)
    if bboxes is None:
        bboxes = torch.tensor([[100., 200., 700., 600.], [0., 0., 1000., 1000.], [300., 100., 500., 900.], [50., 60., 950., 940.],
                               [400., 400., 600., 600.]])[:n]
    files = dict(bboxes=bboxes, betas=torch.randn(n, 10, generator=g), estimated_translation=torch.randn(n, 3, generator=g),
                 gt_j2d=torch.rand(n, 17, 2, generator=g) * 1000, gt_j3d=torch.randn(n, 17, 3, generator=g) * 300,
                 intrinsics=T(ic.small_intrinsics(n)), orient=torch.randn(n, 1, 6, generator=g), pose=torch.randn(n, 23, 6, generator=g))
    for k, v in files.items():
        torch.save(v, str(loc / f'{k}.pt'))
    return loc, files


def test_dataset_image_keys(tmp_path):
    """data_set(..., frames=ArrayFrameSource(...)) follows scripts/data.py:110-158"""
    d = _mod('data')
    n = 4
    loc, files = _write_split(tmp_path, n)
    rs = np.random.RandomState(5)
    frames = [ic.noise_frame(1002, 1000, 50), ic.noise_frame(120, 160, 51), ic.smooth_frame(120, 160), ic.noise_frame(97, 131, 52)]
    masks = [rs.randint(0, 256, size=(224, 224)).astype(np.uint8) for _ in range(n)]
    masks[0][0, 0], masks[1] = 0, masks[0].copy()
    masks[1][0, 0] = 9                                     # masks 0 and 1 differ in pixel [0, 0] only
    plain = d.data_set('validation', root=str(tmp_path))
    ds = d.data_set('validation', root=str(tmp_path), frames=d.ArrayFrameSource(frames, masks))
    assert set(plain[0]) == {'bboxes', 'betas', 'cam', 'gt_j2d', 'gt_j3d', 'intrinsics', 'orient', 'pose', 'inc_gt'}
    reference_keys = {'bboxes', 'betas', 'cam', 'gt_j2d', 'gt_j3d', 'valid', 'mask_rcnn', 'image', 'spin_image', 'intrinsics', 'orient',
                      'pose', 'inc_gt'}                       # scripts/data.py:140-158
    for i in range(n):
        s = ds[i]
        assert set(s) == reference_keys == set(d.REFERENCE_KEYS)
        assert s['spin_image'].shape == (3, 224, 224) and s['image'].shape == (3, 256, 256) and s['mask_rcnn'].shape == (1, 224, 224)
        assert torch.equal(s['gt_j2d'], plain[i]['gt_j2d'])
        assert not s['mask_rcnn'][:, :2, :2].any()
        want = T(masks[i]).float()[None] / 255.0
        want[:, :2, :2] = 0
        assert torch.equal(s['mask_rcnn'], want)
        image = to_image(frames[i])
        crop, _, _, _, k = d.find_crop(image, files['bboxes'][i:i + 1], files['intrinsics'][i:i + 1])
        assert torch.equal(s['image'], crop[0]) and torch.equal(s['intrinsics'], k[0])
        assert torch.equal(s['spin_image'], d.find_crop(image, files['bboxes'][i:i + 1], files['intrinsics'][i:i + 1], img_size=224)[0][0])
    # `valid` is read BEFORE the corner is zeroed
    assert bool(ds[0]['valid']) is False and bool(ds[1]['valid']) is True and torch.equal(ds[0]['mask_rcnn'], ds[1]['mask_rcnn'])
    # the 1002 x 1000 frame is cut to 1000 x 1000 first: rows 1000 and 1001 never matter, and the grid spans 1000 rows
    taller = frames[0].copy()
    taller[1000:] = 255 - taller[1000:]
    ds2 = d.data_set('validation', root=str(tmp_path), frames=d.ArrayFrameSource([taller] + frames[1:], masks))
    assert torch.equal(ds2[0]['image'], ds[0]['image'])
    assert not torch.equal(d.find_crop(T(frames[0]).permute(2, 0, 1).float() / 255.0, files['bboxes'][:1], files['intrinsics'][:1])[0][0],
                           ds[0]['image'])
    # a DataLoader stacks them
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=n)))
    assert batch['image'].shape == (n, 3, 256, 256) and batch['valid'].tolist() == [False, True, bool(masks[2][0, 0]), bool(masks[3][0, 0])]
    # the .npy source reads the same samples; the HDF5 branch says that it is not built
    for i in range(n):
        np.save(loc / f'frame_{i:06d}.npy', frames[i])
        np.save(loc / f'mask_{i:06d}.npy', masks[i])
    src = d.frame_source_for(str(loc))
    assert isinstance(src, d.ArrayFrameSource) and np.array_equal(src.read(2)[0], frames[2]) and np.array_equal(src.read(2)[1], masks[2])
    with pytest.raises(NotImplementedError, match='h5py'):
        d.data_set('validation', root=str(tmp_path), compute_canada=True)
    with pytest.raises(ValueError, match='uint8'):
        d.ArrayFrameSource([frames[0].astype(np.float32)], masks[:1]).read(0)


def test_file_frame_source_reads_image_files(tmp_path):
    """paths from images.pkl, the mask beside it under maskSequence (scripts/data.py:110-118), decoded with PIL"""
    import pickle
    from PIL import Image
    d = _mod('data')
    frame, mask = ic.noise_frame(40, 56, 3), np.random.RandomState(4).randint(0, 256, size=(224, 224)).astype(np.uint8)
    for sub in ('imageSequence', 'maskSequence'):
        (tmp_path / 'S9' / sub / 'cam0').mkdir(parents=True)
    path = tmp_path / 'S9' / 'imageSequence' / 'cam0' / 'img_000001.png'
    Image.fromarray(frame).save(path)
    Image.fromarray(mask).save(tmp_path / 'S9' / 'maskSequence' / 'cam0' / 'img_000001.png')
    with open(tmp_path / 'images.pkl', 'wb') as f:
        pickle.dump(np.array([str(path)]), f)
    got = d.FileFrameSource(str(tmp_path)).read(0)
    assert np.array_equal(got[0], frame) and np.array_equal(got[1], mask)


def test_region_of_interest_holds_every_tap():
    """for 1 000 seeded bboxes (a third partly outside the frame): the block crop_roi names contains every in-frame tap of non-zero
    weight of both crops, and find_crop on the block alone equals find_crop on the whole frame exactly"""
    d = _mod('data')
    H, W = 230, 310
    image = to_image(ic.noise_frame(H, W, 77))
    bbs = T(ic.roi_bboxes())
    assert bbs.shape == (1000, 4)
    partly = ((bbs[:, :2] < 0).any(1) | (bbs[:, 2:] > 1000).any(1))
    assert 250 < int(partly.sum()) < 420
    rois = d.crop_roi(bbs, H, W, sizes=(32, 48))
    ax, ay, scale = d._crop_centres(bbs)
    saved = 0
    for n in (32, 48):
        for (centre, extent, lo, size) in ((ay, H, rois[:, 0], rois[:, 2]), (ax, W, rois[:, 1], rois[:, 3])):
            i0, w0, w1 = d.axis_taps(scale, centre, n, extent)
            assert ((w0 == 0) | ((i0 >= 0) & (i0 < extent))).all() and ((w1 == 0) | ((i0 + 1 >= 0) & (i0 + 1 < extent))).all()
            assert ((w0 == 0) | ((i0 >= lo[:, None]) & (i0 < (lo + size)[:, None]))).all()
            assert ((w1 == 0) | ((i0 + 1 >= lo[:, None]) & (i0 + 1 < (lo + size)[:, None]))).all()
    k = torch.eye(3)[None]
    for b in range(0, 1000):
        y0, x0, h, w = rois[b].tolist()
        assert 0 <= y0 and y0 + h <= H and 0 <= x0 and x0 + w <= W
        saved += H * W - h * w
        for n in (32, 48):
            whole = d.find_crop(image, bbs[b:b + 1], k, img_size=n)[0]
            block = d.find_crop(image[:, y0:y0 + h, x0:x0 + w], bbs[b:b + 1], k, img_size=n, roi=(y0, x0, H, W))[0]
            assert torch.equal(whole, block), b
    assert saved > 0.3 * 1000 * H * W                        # the blocks are smaller than the frames
    # a block one row short is refused, not sampled wrongly
    b = int(torch.nonzero(rois[:, 2] > 2)[0])
    y0, x0, h, w = rois[b].tolist()
    with pytest.raises(ValueError, match='region of interest'):
        d.find_crop(image[:, y0:y0 + h - 1, x0:x0 + w], bbs[b:b + 1], k, img_size=48, roi=(y0, x0, H, W))


def test_pack_frames_descriptors():
    d = _mod('data')
    frames = [ic.noise_frame(20, 30, 1), ic.noise_frame(17, 13, 2)]
    rois = torch.tensor([[2, 3, 10, 7], [0, 0, 17, 13]])
    pix, desc = d.pack_frames(frames, rois)
    assert pix.dtype == torch.uint8 and pix.numel() % 16 == 0 and desc.dtype == torch.int64 and desc.shape == (2, 8)
    for f, r, row in zip(frames, rois.tolist(), desc.tolist()):
        off, pitch, y0, x0, h, w, H, W = row
        assert off % 16 == 0 and pitch == 3 * w and [y0, x0, h, w] == r and (H, W) == f.shape[:2]
        assert np.array_equal(pix[off:off + h * pitch].numpy().reshape(h, w, 3), f[y0:y0 + h, x0:x0 + w])


def test_image_entry_points_refuse_bad_arguments():
    """negative status + message before anything touches the device (no GPU needed)"""
    import ctypes
    _mod('build').build(verbose=False)
    lib = _mod('_lib').load()
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails its argument check
    for s0, s1 in ((30, 0), (260, 0), (224, 258), (0, 0), (224, -4)):
        assert lib.jrr_image_crop(p, 4096, p, p, 2, None, None, s0, p, s1, p, p, None) == -1
        assert b'multiples of 4' in lib.jrr_last_error()
    assert lib.jrr_image_crop(p, 4096, p, p, 2, None, None, 224, p, 256, None, p, None) == -1      # second size without its output
    assert lib.jrr_image_crop(p, 4096, p, p, 2, p, None, 224, p, 0, None, p, None) == -1           # mean without std
    assert lib.jrr_image_crop(p, 4100, p, p, 2, None, None, 224, p, 0, None, p, None) == -1 and b'16' in lib.jrr_last_error()
    assert lib.jrr_image_crop(p, 4096, p, p, 2, None, None, 224, p, 0, None, None, None) == -1     # no status word
    assert lib.jrr_mask_prepare(p, 2, 0, 224, p, p, None) == -1 and b'jrr_mask_prepare' in lib.jrr_last_error()
    assert lib.jrr_image_crop(p, 4096, p, p, 0, None, None, 224, p, 256, p, p, None) == 0          # an empty batch launches nothing


def test_image_masks_flag():
    a = _mod('args')
    assert a.get_args([]).image_masks is False
    assert a.get_args(['--silhouette', '--image_masks', '--data_root', 'x']).image_masks is True
    for k, v in a.REFERENCE_FLAGS.items():
        assert getattr(a.get_args(['--image_masks']), k) == v
