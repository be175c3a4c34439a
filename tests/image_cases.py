"""Inputs of the image-pipeline checks, defined ONCE from seeds for the golden generator (tests/golden/make_golden_images.py) and for
the tests (tests/test_image_pipeline.py, tests/test_gpu_image_pipeline.py).  numpy.random.RandomState is stable across numpy versions.

Bounding boxes are (min_y, min_x, max_y, max_x) in the reference's 1000-unit frame convention whatever the frame's real size
(scripts/data.py:220-247: the sampling grid spans the whole frame)."""
import numpy as np


def noise_frame(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def smooth_frame(h, w):
    """two smooth channels and a 16-px checker of 0 / 255: full-range jumps between neighbours, the hardest case for a position error"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    c0 = 127.5 + 127.5 * np.sin(x / w * 2 * np.pi) * np.cos(y / h * np.pi)
    c1 = 255.0 * (x + 2 * y) / (w + 2 * h)
    c2 = 255.0 * (((x // 16) + (y // 16)) % 2)
    return np.stack([c0, c1, c2], -1).round().astype(np.uint8)


def small_frames():
    return {'noise': noise_frame(120, 160, 11), 'smooth': smooth_frame(120, 160), 'odd': noise_frame(97, 131, 12)}


# (name, frames of the batch, bboxes of the batch, crop size)
SMALL_CASES = [
    ('inside_32', ['noise'], [[200., 300., 700., 800.]], 32),
    ('inside_48', ['noise'], [[200., 300., 700., 800.]], 48),
    ('full_32', ['noise'], [[0., 0., 1000., 1000.]], 32),
    ('full_48', ['smooth'], [[0., 0., 1000., 1000.]], 48),
    ('wide_48', ['smooth'], [[400., 100., 600., 900.]], 48),
    ('tall_32', ['smooth'], [[100., 400., 900., 600.]], 32),
    ('partly_low_48', ['odd'], [[-400., -400., 100., 100.]], 48),
    ('partly_high_32', ['noise'], [[900., 900., 1500., 1500.]], 32),
    ('outside_32', ['noise'], [[1200., 1200., 1500., 1500.]], 32),
    ('tiny_48', ['smooth'], [[450., 450., 520., 500.]], 48),
    ('tiny_odd_32', ['odd'], [[450., 450., 520., 500.]], 32),
    ('zero_size_32', ['noise'], [[300., 300., 300., 300.]], 32),
    ('batch2_32', ['noise', 'smooth'], [[150., 250., 650., 700.], [420., 380., 640., 460.]], 32),
]
ALL_ZERO_CASES = ('outside_32', 'zero_size_32')
ZERO_SIZE_CASES = ('zero_size_32',)


def small_intrinsics(n):
    """a plausible pinhole matrix per sample (Human3.6M cameras: focal ~1145 px, centre ~ (512, 515))"""
    k = np.zeros((n, 3, 3), np.float32)
    for i in range(n):
        k[i] = [[1145.0 + 3 * i, 0, 512.5 - i], [0, 1143.8 - 2 * i, 515.4 + i], [0, 0, 1]]
    return k


LARGE_H, LARGE_W = 1002, 1000        # cut to 1000 x 1000 before cropping (scripts/data.py:111-112)


def large_frames():
    return {'noise': noise_frame(LARGE_H, LARGE_W, 21), 'smooth': smooth_frame(LARGE_H, LARGE_W)}


def large_bboxes():
    """37 seeded bboxes of the classes of SMALL_CASES"""
    rs = np.random.RandomState(31)
    out = []
    for k in range(37):
        cls = k % 7
        if k == 35:                                   # wholly outside
            bb = [1150., -900., 1700., -300.]
        elif k == 36:                                 # zero size
            bb = [412., 633., 412., 633.]
        elif cls == 0:                                # inside
            cy, cx, h = rs.uniform(300, 700), rs.uniform(300, 700), rs.uniform(100, 280)
            bb = [cy - h, cx - 0.6 * h, cy + h, cx + 0.6 * h]
        elif cls == 1:                                # (nearly) the full frame
            e = rs.uniform(0, 3)
            bb = [e, e, 1000. - e, 1000. - e] if k > 1 else [0., 0., 1000., 1000.]
        elif cls == 2:                                # wider than tall
            cy, cx = rs.uniform(300, 700), rs.uniform(450, 550)
            bb = [cy - 80, cx - 400, cy + 80, cx + 400]
        elif cls == 3:                                # taller than wide
            cy, cx = rs.uniform(450, 550), rs.uniform(300, 700)
            bb = [cy - 420, cx - 60, cy + 420, cx + 60]
        elif cls == 4:                                # partly outside, low corner
            a, s = rs.uniform(-500, -50), rs.uniform(300, 700)
            bb = [a, a + 30, a + s, a + 30 + 0.8 * s]
        elif cls == 5:                                # partly outside, high corner
            a, s = rs.uniform(700, 950), rs.uniform(300, 700)
            bb = [a, a - 20, a + s, a - 20 + 0.9 * s]
        else:                                         # tiny: strong magnification
            cy, cx = rs.uniform(100, 900), rs.uniform(100, 900)
            bb = [cy - rs.uniform(5, 40), cx - rs.uniform(5, 40), cy + rs.uniform(5, 40), cx + rs.uniform(5, 40)]
        out.append(bb)
    return np.asarray(out, np.float32)


def roi_bboxes(n=1000, seed=41):
    """seeded bboxes of the ROI property test: a third of them partly outside the frame"""
    rs = np.random.RandomState(seed)
    cy, cx = rs.uniform(100, 900, n), rs.uniform(100, 900, n)
    hh = rs.uniform(0.02, 0.98, n) * np.minimum(cy, 1000 - cy)          # inside the frame ...
    hw = rs.uniform(0.02, 0.98, n) * np.minimum(cx, 1000 - cx)
    out = rs.rand(n) < 1 / 3                                            # ... except a third: the centre near or beyond an edge
    cy = np.where(out, np.where(rs.rand(n) < 0.5, rs.uniform(-100, 60, n), rs.uniform(940, 1100, n)), cy)
    cx = np.where(out & (rs.rand(n) < 0.5), rs.uniform(-100, 1100, n), cx)
    hh, hw = np.where(out, rs.uniform(110, 450, n), hh), np.where(out, rs.uniform(30, 450, n), hw)
    return np.stack([cy - hh, cx - hw, cy + hh, cx + hw], 1).astype(np.float32)
