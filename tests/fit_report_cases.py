"""Host restatement of the fit report and the inputs its tests share (tests/test_fit_report.py, tests/test_gpu_fit_report.py).

Written from the reference's lines, not from the kernels: viz() of /root/reference/scripts/optimize.py:28-74

    render    = torch.where(render > 0.5, ones, zeros)           :35-36
    mask_rcnn = torch.where(mask_rcnn > 0.8, ones, zeros)        :41-42
    torch.where(mask_rcnn + render == 1, ones, zeros)            :47-48   (the disagreement map that is shown)
    plt.imshow(...); plt.scatter(joints[:, 0], joints[:, 1])     :61-64   (pixel (x, y) is centred AT the integer coordinate)

and from the arithmetic include/jrr.h fixes for the picture.  The comparisons are torch's on float32 tensors: the threshold is
rounded to float32 first, so mask byte 204 (204 / 255 = 0.800000012 in float32 = float32(0.8)) is NOT mask and 205 is the first
that is; a float64 comparison would count 204 in.
"""
import struct
import zlib

import numpy as np
import torch

F = np.float32
TINT = {(True, False): (255, 0, 0), (False, True): (0, 0, 255), (True, True): (0, 255, 0)}       # (render, mask) -> colour
SET_COLOURS = ((0, 255, 0), (255, 255, 0), (255, 0, 255))


def binarise(x, thr):
    """torch.where(x > thr, ones, zeros) on a float32 tensor, as the reference writes it -> bool numpy array"""
    t = torch.as_tensor(np.asarray(x, dtype=F))
    return torch.where(t > thr, torch.ones_like(t), torch.zeros_like(t)).numpy() == 1


def compare_ref(alpha, mask, thr_render=0.5, thr_mask=0.8):
    """(B,h,w) float32 arrays -> int32 (B,4) = {r & m, r | m, r, m} pixel counts"""
    r, m = binarise(alpha, thr_render), binarise(mask, thr_mask)
    B = r.shape[0]
    return np.stack([(r & m).reshape(B, -1).sum(1), (r | m).reshape(B, -1).sum(1), r.reshape(B, -1).sum(1), m.reshape(B, -1).sum(1)],
                    1).astype(np.int32)


def iou_ref(alpha, mask, thr_render=0.5, thr_mask=0.8):
    c = compare_ref(alpha, mask, thr_render, thr_mask).astype(np.float64)
    return np.where(c[:, 1] > 0, c[:, 0] / np.maximum(c[:, 1], 1), 1.0)


def overlay_ref(alpha, mask, image=None, normalize=None, joints2d=(), radius=2.0, thr_render=0.5, thr_mask=0.8):
    """uint8 (B,S,S,3), every operation in float32 and rounded once"""
    alpha, mask = np.asarray(alpha, dtype=F), np.asarray(mask, dtype=F)
    B, S, _ = alpha.shape
    if image is None:
        bg = np.zeros((B, S, S, 3), dtype=np.int64)
    else:
        x = np.asarray(image, dtype=F)
        if normalize is not None:
            mean, std = (np.asarray(v, dtype=F).reshape(1, 3, 1, 1) for v in normalize)
            x = (x * std).astype(F) + mean
        x = np.fmin(np.fmax(x, F(0)), F(1))                       # fmaxf / fminf
        bg = np.floor((x * F(255)).astype(F) + F(0.5)).astype(np.int64).transpose(0, 2, 3, 1)
    r, m = binarise(alpha, thr_render), binarise(mask, thr_mask)
    out = bg.copy()
    for (fr, fm), colour in TINT.items():
        sel = (r == fr) & (m == fm)
        out[sel] = (bg[sel] + np.asarray(colour, dtype=np.int64) + 1) >> 1
    xs, ys = np.arange(S, dtype=F)[None, :], np.arange(S, dtype=F)[:, None]
    r2 = F(radius) * F(radius)
    for s, joints in enumerate(joints2d):
        joints = np.asarray(joints, dtype=F)
        for b in range(B):
            for jx, jy in joints[b]:
                if not (np.isfinite(jx) and np.isfinite(jy)):
                    continue
                dx, dy = xs - jx, ys - jy
                out[b][(dx * dx).astype(F) + (dy * dy).astype(F) <= r2] = SET_COLOURS[s]
    return out.astype(np.uint8)


# ---- a PNG reader for what report.write_png writes (8-bit RGB, filter 0), standard library only ----
def read_png(path):
    """-> (array (H,W,3) uint8, chunk tags); asserts the signature, every CRC, the IHDR fields and the filter bytes"""
    raw = open(path, 'rb').read()
    assert raw[:8] == b'\x89PNG\r\n\x1a\n'
    pos, chunks = 8, []
    while pos < len(raw):
        n, tag = struct.unpack('>I4s', raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack('>I', raw[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + data) & 0xffffffff, tag
        chunks.append((tag, data))
        pos += 12 + n
    tags = [t for t, _ in chunks]
    assert tags[0] == b'IHDR' and tags[-1] == b'IEND' and b'IDAT' in tags
    w, h, depth, colour, comp, filt, interlace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(b''.join(d for t, d in chunks if t == b'IDAT')), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any()                                # filter type 0 on every scanline
    return rows[:, 1:].reshape(h, w, 3).copy(), tags


# ---- shared inputs ----
def compare_case(B, h, w, seed=0):
    """alpha, mask (B,h,w) float32.  Pose 0: seeded random alpha with planted 0.5 / nextafter(0.5, 1) / NaN / +-inf and a mask of
    uint8 / 255 running through all 256 byte values (204 and 205 first); pose 1 (B >= 2): both empty; pose 2: both full."""
    rng = np.random.RandomState(1000 * seed + h * 7 + w)
    n = h * w
    alpha = rng.uniform(-0.2, 1.2, size=(B, n)).astype(F)
    planted = np.array([0.5, np.nextafter(F(0.5), F(1)), np.nextafter(F(0.5), F(0)), np.nan, np.inf, -np.inf], dtype=F)
    alpha[0, rng.permutation(n)[:len(planted)]] = planted
    byte = (np.arange(n) + 204) % 256
    mask = np.tile((byte.astype(np.uint8).astype(F) / F(255))[None], (B, 1))
    if n > 256:
        mask[0, 256:] = rng.randint(0, 256, size=n - 256).astype(np.uint8).astype(F) / F(255)
    if B >= 2:
        alpha[1], mask[1] = 0, 0
    if B >= 3:
        alpha[2], mask[2] = 1, 1
    return alpha.reshape(B, h, w), mask.reshape(B, h, w)


def overlay_case(B, S, n_sets, with_image, radius, seed=0):
    """alpha, mask (B,S,S), image (B,3,S,S) or None, joint sets [n_sets] of (B,17,2).  Joint coordinates and the radius are multiples
    of 1/4: dx * dx + dy * dy is exact in float32 however it is evaluated.  Planted: joints at two corners, one with a pixel at exactly
    `radius` along x (its coordinates chosen so that x + radius is an integer), (-1,-1), S + 5, NaN, +-inf; image values exactly 0, 1,
    -0.25, 1.5 among k / 255."""
    rng = np.random.RandomState(77 * seed + 13 * S + B + 5 * n_sets)
    alpha = rng.uniform(0, 1, size=(B, S, S)).astype(F)
    alpha[:, 0, 0], alpha[:, 0, 1] = 0.5, np.nextafter(F(0.5), F(1))
    mask = rng.randint(0, 256, size=(B, S, S)).astype(np.uint8).astype(F) / F(255)
    mask[:, 1, 0], mask[:, 1, 1] = F(204) / F(255), F(205) / F(255)
    image = None
    if with_image:
        image = rng.randint(0, 256, size=(B, 3, S, S)).astype(np.uint8).astype(F) / F(255)
        image[:, :, 2, 0], image[:, :, 2, 1], image[:, :, 2, 2], image[:, :, 2, 3] = 0.0, 1.0, -0.25, 1.5
    sets = []
    for s in range(n_sets):
        j = (rng.randint(-12, 4 * S + 12, size=(B, 17, 2)) / 4.0).astype(F)
        frac = F(radius) - np.floor(F(radius))
        j[:, 0] = (0, 0)
        j[:, 1] = (S - 1, S - 1)
        j[:, 2] = (F(S // 2) - frac, S // 2)                    # pixel (S/2 - frac + radius, S/2) lies exactly on the rim
        j[:, 3] = (-1, -1)
        j[:, 4] = (S + 5, S + 5)
        j[:, 5] = (np.nan, 1)
        j[:, 6] = (1, np.inf)
        j[:, 7] = (-np.inf, np.nan)
        j[:, 8] = (S - 1, 0.25)
        sets.append(j)
    return alpha, mask, image, sets
