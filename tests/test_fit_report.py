"""The fit report without a GPU: the C ABI rows, the PNG writer, the host restatement against cases worked by hand, the flags.

(--fit_report: /root/reference/scripts/optimize.py:204-218,268-274 and viz() at :28-74.)"""
import importlib
import os
import re
import struct
import zlib

import numpy as np
import pytest

import fit_report_cases as frc
from conftest import PKG_NAME, ROOT

F = np.float32


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def test_report_symbols_declared_exported_and_in_the_table():
    hdr = open(os.path.join(ROOT, 'include', 'jrr.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    lib_mod = _mod('_lib')
    _mod('build').build(verbose=False)
    lib = lib_mod.load()
    for name in ('jrr_silhouette_compare', 'jrr_fit_overlay'):
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in lib_mod.SIGNATURES and hasattr(lib, name), name
        assert re.search(r'\|[^|\n]*`' + name + r'`[^|\n]*\|[^\n]*scripts/optimize\.py', doc), name      # a table row with a call site
    assert all(s in hdr for s in ('scripts/optimize.py:35-48', '204-218', '268-274'))      # the lines the two functions replace
    assert 'report.hip' in _mod('build').SOURCES
    # argument errors come back as a status, nothing is launched (no device is touched: the pointers are never read)
    import ctypes
    p = ctypes.c_void_p(4096)
    assert lib.jrr_silhouette_compare(p, p, 2, 5, 3, 0.5, 0.8, p, None) == -1 and b'multiple of 4' in lib.jrr_last_error()
    assert lib.jrr_silhouette_compare(p, None, 2, 4, 4, 0.5, 0.8, p, None) == -1
    assert lib.jrr_silhouette_compare(p, p, 0, 4, 4, 0.5, 0.8, p, None) == 0                        # an empty batch launches nothing
    assert lib.jrr_fit_overlay(p, p, None, None, None, None, 0, 2, 6, 0.5, 0.8, 2.0, p, None) == -1 and b'size 6' in lib.jrr_last_error()
    assert lib.jrr_fit_overlay(p, p, None, None, None, None, 0, 2, 260, 0.5, 0.8, 2.0, p, None) == -1
    assert lib.jrr_fit_overlay(p, p, None, None, None, None, 4, 2, 224, 0.5, 0.8, 2.0, p, None) == -1      # more than three joint sets
    assert lib.jrr_fit_overlay(p, p, None, None, None, None, 1, 2, 224, 0.5, 0.8, 2.0, p, None) == -1      # a set without its joints
    assert lib.jrr_fit_overlay(p, p, p, p, None, None, 0, 2, 224, 0.5, 0.8, 2.0, p, None) == -1           # mean without std
    assert lib.jrr_fit_overlay(p, p, None, None, None, None, 0, 0, 224, 0.5, 0.8, 2.0, p, None) == 0


@pytest.mark.parametrize('h,w', [(5, 3), (224, 224)])
def test_write_png_bytes(tmp_path, h, w):
    """signature, IHDR, CRCs and the inflated scanlines, checked with zlib / struct alone"""
    report = _mod('report')
    rgb = np.random.RandomState(h).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    path = str(tmp_path / 'a.png')
    report.write_png(path, rgb)
    raw = open(path, 'rb').read()
    assert raw[:8] == b'\x89PNG\r\n\x1a\n'
    assert raw[8:16] == struct.pack('>I', 13) + b'IHDR' and raw[16:29] == struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)
    assert raw[29:33] == struct.pack('>I', zlib.crc32(raw[12:29]) & 0xffffffff)
    assert raw[-12:] == struct.pack('>I', 0) + b'IEND' + struct.pack('>I', zlib.crc32(b'IEND') & 0xffffffff)
    back, tags = frc.read_png(path)                             # every chunk's CRC, filter byte 0 per scanline
    assert tags == [b'IHDR', b'IDAT', b'IEND'] and np.array_equal(back, rgb)
    import torch
    report.write_png(path, torch.from_numpy(rgb))               # a tensor as well
    assert np.array_equal(frc.read_png(path)[0], rgb)
    for bad in (rgb[..., :2], rgb.astype(np.int32), rgb[0]):
        with pytest.raises(ValueError):
            report.write_png(path, bad)


def test_write_png_round_trip_through_pil(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    rgb = np.random.RandomState(3).randint(0, 256, size=(7, 12, 3)).astype(np.uint8)
    path = str(tmp_path / 'b.png')
    _mod('report').write_png(path, rgb)
    with Image.open(path) as im:
        assert im.mode == 'RGB' and im.size == (12, 7) and np.array_equal(np.asarray(im), rgb)


def test_restatement_mask_bytes_204_and_205():
    """torch compares a float32 tensor with float32(0.8): 204 / 255 rounds to exactly that and is not mask, 205 / 255 is"""
    assert F(204) / F(255) == F(0.8) and float(F(204) / F(255)) > 0.8           # ... which a float64 comparison would count in
    mask = np.zeros((1, 4, 4), dtype=F)
    mask[0, 0, 0], mask[0, 0, 1], mask[0, 3, 3] = F(204) / F(255), F(205) / F(255), 1.0
    alpha = np.zeros((1, 4, 4), dtype=F)
    alpha[0, 0, 0], alpha[0, 0, 1], alpha[0, 2, 2] = 1.0, 0.5, np.nextafter(F(0.5), F(1))
    alpha[0, 1, :] = (np.nan, np.inf, -np.inf, 0.75)
    # render: (0,0), (2,2), (1,1), (1,3); mask: (0,1), (3,3); no pixel in both
    assert frc.compare_ref(alpha, mask).tolist() == [[0, 6, 4, 2]]
    assert frc.iou_ref(alpha, mask).tolist() == [0.0]
    mask[0, 0, 0] = F(205) / F(255)
    assert frc.compare_ref(alpha, mask).tolist() == [[1, 6, 4, 3]]
    z = np.zeros((2, 4, 4), dtype=F)
    assert frc.iou_ref(z, z).tolist() == [1.0, 1.0]                              # both empty: they agree
    iou = _mod('report').iou_from_counts
    import torch
    got = iou(torch.tensor([[1, 6, 4, 3], [0, 0, 0, 0], [16, 16, 16, 16]], dtype=torch.int32))
    assert got.dtype == torch.float64 and got.tolist() == [1 / 6, 1.0, 1.0]


def test_restatement_tint_table():
    alpha = np.zeros((1, 4, 4), dtype=F)
    mask = np.zeros((1, 4, 4), dtype=F)
    alpha[0, 0, 1] = alpha[0, 0, 3] = 1.0          # (y 0, x 1): render only; (0, 3): both
    mask[0, 0, 2] = mask[0, 0, 3] = 1.0            # (0, 2): mask only
    image = np.zeros((1, 3, 4, 4), dtype=F)
    image[0, :, 0, :] = np.array([100, 50, 201], dtype=F)[:, None] / F(255)
    image[0, 0, 1, :] = (0.0, 1.0, -0.25, 1.5)     # clamped: 0, 255, 0, 255
    image[0, 1, 1, :] = (F(0.5), F(127.4) / F(255), F(1) / F(510), F(254.5) / F(255))
    out = frc.overlay_ref(alpha, mask, image)
    assert out.shape == (1, 4, 4, 3) and out.dtype == np.uint8
    assert out[0, 0, 0].tolist() == [100, 50, 201]                               # neither: the background
    assert out[0, 0, 1].tolist() == [(100 + 255 + 1) >> 1, (50 + 1) >> 1, (201 + 1) >> 1] == [178, 25, 101]
    assert out[0, 0, 2].tolist() == [50, 25, (201 + 255 + 1) >> 1] == [50, 25, 228]
    assert out[0, 0, 3].tolist() == [50, (50 + 255 + 1) >> 1, 101] == [50, 153, 101]
    assert out[0, 1, :, 0].tolist() == [0, 255, 0, 255]
    assert out[0, 1, 0, 1] == 128 and out[0, 1, 1, 1] == 127                     # 127.5 rounds up (half up), 127.4 down
    assert out[0, 2:].max() == 0
    # without an image the background is black; SPIN's normalisation is undone as x * std + mean
    assert frc.overlay_ref(alpha, mask)[0, 0].tolist() == [[0, 0, 0], [128, 0, 0], [0, 0, 128], [0, 128, 0]]
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    norm = ((image - np.asarray(mean, dtype=F).reshape(1, 3, 1, 1)) / np.asarray(std, dtype=F).reshape(1, 3, 1, 1)).astype(F)
    assert np.abs(frc.overlay_ref(alpha, mask, norm, (mean, std)).astype(int) - out.astype(int)).max() <= 1


def test_restatement_disc_of_radius_one_at_a_corner():
    z = np.zeros((1, 4, 4), dtype=F)
    nan = np.full((1, 17, 2), np.nan, dtype=F)
    a, b = nan.copy(), nan.copy()
    a[0, 0] = (0, 0)                               # the corner: itself and its two neighbours, clipped
    a[0, 1] = (np.inf, 1)
    b[0, 3] = (1, 0)                               # the later set wins where both cover
    b[0, 4] = (3.5, 3.5)                           # between four pixel centres: only (3,3) exists, at 0.707
    b[0, 5] = (-1, -1)                             # (0,0) is at 1.41: nothing
    out = frc.overlay_ref(z, z, joints2d=[a, b], radius=1.0)
    want = np.zeros((4, 4, 3), dtype=np.uint8)
    for (y, x) in ((0, 0), (0, 1), (1, 0)):
        want[y, x] = (0, 255, 0)
    for (y, x) in ((0, 0), (0, 1), (0, 2), (1, 1), (3, 3)):
        want[y, x] = (255, 255, 0)
    assert np.array_equal(out[0], want)
    three = frc.overlay_ref(z, z, joints2d=[nan, nan, a], radius=1.0)[0]
    assert three[0, 0].tolist() == [255, 0, 255] and (three.reshape(-1, 3).any(1).sum() == 3)


def test_fit_report_needs_silhouette():
    argsmod, opt = _mod('args'), _mod('optimize')
    saved = argsmod._LazyArgs._ns
    try:
        argsmod._LazyArgs._ns = argsmod.get_args(['--fit_report', 'somewhere', '--synthetic'])
        with pytest.raises(ValueError, match='--fit_report needs --silhouette'):
            opt.optimize_pose_refiner(log=lambda r: None)
    finally:
        argsmod._LazyArgs._ns = saved


def test_fit_report_flags_and_reference_defaults():
    a = _mod('args')
    ns = a.get_args([])
    assert ns.fit_report is None and ns.fit_report_images == 8
    ns = a.get_args(['--silhouette', '--fit_report', 'out', '--fit_report_images', '3'])
    assert ns.fit_report == 'out' and ns.fit_report_images == 3
    assert len(a.REFERENCE_FLAGS) == 15
    for k, v in a.REFERENCE_FLAGS.items():
        assert getattr(ns, k) == v, k
