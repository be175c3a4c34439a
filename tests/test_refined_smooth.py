"""The time-axis filter over the refined-pose table without a GPU: the runs of consecutive frames (refined.sequence_runs), the properties
of the float64 restatement (tests/refined_smooth_cases.py) and its float32 yardsticks, the C ABI rows, the refined_smooth.npz /
meta.json files through refined.smooth with the three operators replaced by the host restatement, the `.npz` form of
`--init_refined`, and the flags."""
import importlib
import json
import os
import pickle
import re

import numpy as np
import pytest
import torch

import refined_cases as rc
import refined_smooth_cases as sc
from conftest import PKG_NAME, ROOT

F = np.float32
T = torch.from_numpy


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _path(action, camera, frame, subject='S9'):
    return f'/data/h36m/{subject}/{action}/imageSequence/{camera}/img_{frame:06d}.jpg'


# ---- 1. runs of consecutive frames ----
def test_sequence_key_and_frame():
    refined = _mod('refined')
    assert refined.sequence_key(_path('Walking 1', '5', 12)) == ('/data/h36m/S9/Walking 1/imageSequence/5', 12)
    assert refined.sequence_key('S9\\Eating\\imageSequence\\c2\\img_000310.png') == ('S9/Eating/imageSequence/c2', 310)
    for bad in ('/data/frames/000012.jpg', '/data/S9/Eating/imageSequence/img_000001.jpg', '/data/S9/Eating/imageSequence/5/frame12.jpg', '', None):
        assert refined.sequence_key(bad) == (None, -1), bad


def test_two_cameras_interleaved_in_file_order():
    refined = _mod('refined')
    paths = [_path('Walking', cam, f) for f in range(1, 7) for cam in ('1', '2')]          # c1 f1, c2 f1, c1 f2, ...
    order, run, frame = refined.sequence_runs(paths, np.ones(12, np.uint8))
    assert order.dtype == np.int32 and run.dtype == np.int32 and frame.dtype == np.int64
    assert order.tolist() == [0, 2, 4, 6, 8, 10, 1, 3, 5, 7, 9, 11] and run.tolist() == [0] * 6 + [1] * 6
    assert frame.tolist() == [1, 2, 3, 4, 5, 6] * 2
    assert sorted(order.tolist()) == list(range(12)) and (np.diff(order) < 0).any()         # a true permutation


def test_gap_duplicate_unrefined_stride_and_strays():
    refined = _mod('refined')
    frames = [5, 10, 15, 25, 30, 30, 35, 40, 45, 50, 55]                                     # stride 5; 20 missing; 30 twice
    paths = [_path('Eating', '3', f) for f in frames] + ['/data/other/frame_07.jpg', _path('Eating', '3', 60), '/data/other/frame_08.jpg']
    has = np.ones(len(paths), np.uint8)
    has[8] = 0                                                                               # frame 45: unrefined in mid-sequence
    order, run, frame = refined.sequence_runs(paths, has)
    assert order.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 12, 11, 13]
    #                       5 10 15 | 25 30 | 30 35 40 | 50 55 60 | stray | stray
    assert run.tolist() == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 5]
    assert frame.tolist() == [5, 10, 15, 25, 30, 30, 35, 40, 50, 55, 60, -1, -1]
    assert (np.diff(run) >= 0).all() and 8 not in order
    # rows are sorted by (key, frame, dataset index): the two rows of frame 30 keep their dataset order
    assert order[4] < order[5]
    # a key with a single refined frame, and nothing refined at all
    o, r, f = refined.sequence_runs([_path('A', '1', 3), _path('B', '1', 9), _path('B', '1', 10)], np.array([1, 1, 1]))
    assert o.tolist() == [0, 1, 2] and r.tolist() == [0, 1, 1] and f.tolist() == [3, 9, 10]
    o, r, f = refined.sequence_runs([_path('A', '1', 3)] * 4, np.zeros(4))
    assert o.shape == r.shape == f.shape == (0,) and o.dtype == np.int32 and f.dtype == np.int64
    with pytest.raises(ValueError, match='3 paths for a table of 4 rows'):
        refined.sequence_runs(['a', 'b', 'c'], np.ones(4))


def test_keys_and_frames_form_agrees_with_paths():
    refined = _mod('refined')
    rng = np.random.RandomState(0)
    cams = rng.randint(0, 3, size=60)
    frames = rng.randint(0, 30, size=60) * 2
    has = (rng.uniform(size=60) < 0.8).astype(np.uint8)
    by_path = refined.sequence_runs([_path('Posing', str(c), f) for c, f in zip(cams, frames)], has)
    by_keys = refined.sequence_runs((cams, frames), has)
    for a, b in zip(by_path, by_keys):
        assert np.array_equal(a, b)
    order, run, frame = by_keys
    assert sorted(order.tolist()) == np.nonzero(has)[0].tolist()
    same = run[1:] == run[:-1]
    assert same.any() and (np.diff(frame)[same] == 2).all() and (cams[order][1:][same] == cams[order][:-1][same]).all()
    # a negative frame in the second form: a run of its own, behind the keyed rows
    o, r, f = refined.sequence_runs((np.array([7, 7, 7, 7]), np.array([1, -1, 2, 3])), np.ones(4))
    assert o.tolist() == [0, 2, 3, 1] and r.tolist() == [0, 0, 0, 1] and f.tolist() == [1, 2, 3, -1]


# ---- 2. properties of the restatement in float64 ----
def _smooth64(x6d, run, radius, sigma=2.0):
    n = x6d.shape[0]
    betas, cam = np.linspace(-1, 1, n * 10).reshape(n, 10), np.linspace(2, 3, n * 3).reshape(n, 3)
    return sc.smooth(x6d, betas, cam, run, sc.weights(sigma, radius)), betas, cam


def test_a_constant_sequence_is_unchanged():
    x = np.repeat(sc.trajectories(1, lengths=(1,))[:1], 9, 0).astype(np.float64)
    (x_out, b_out, c_out, delta), betas, cam = _smooth64(x, np.zeros(9, int), 3)
    assert sc.dist_rot(x_out, x) <= 1e-14 and np.abs(delta).max() <= 1e-6          # atan2 of a 1e-16 residual: 1e-8 rad at most
    assert np.nanmax(np.abs(sc.jitter(x, np.zeros(9, int))[1:-1])) <= 1e-5
    const = np.ones((9, 10))
    assert np.abs(sc.smooth(x, const, const[:, :3], np.zeros(9, int), sc.weights(2.0, 3))[1] - 1).max() <= 1e-15


def test_constant_angular_velocity_keeps_interior_positions_and_has_zero_jitter():
    Tn, radius = 21, 4
    x = np.stack([sc.constant_velocity(Tn, (1, 2, 3), 0.3, 0.07), sc.constant_velocity(Tn, (0, -1, 1), 2.0, -0.11)], 1)
    (x_out, _, _, delta), _, _ = _smooth64(x, np.zeros(Tn, int), radius)
    inner = slice(radius, Tn - radius)
    assert sc.dist_rot(x_out[inner], x[inner]) <= 1e-14 and np.abs(delta[inner]).max() <= 1e-6
    assert delta[0] > 0.1 and delta[-1] > 0.1                                       # the truncated windows at the ends do move
    jit = sc.jitter(x, np.zeros(Tn, int))
    assert np.isnan(jit[[0, -1]]).all() and np.abs(jit[1:-1]).max() <= 1e-5


def test_negating_every_other_quaternion_changes_nothing():
    """q and -q are one rotation: the filter must not see which one Shepperd's branch happened to return.  The sequence crosses w = 0, so
    the branch differs between neighbours; negating every other frame's quaternion before the sum gives the same bits."""
    Tn = 25
    x = sc.sign_crossing(Tn)[:, None, :]
    R = sc.rot6d(x)[:, 0]
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    by_trace = tr >= np.max([R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]], 0)
    w0 = sc.unit_quat(sc.rot6d(x))[:, 0, 0]
    assert by_trace.any() and not by_trace.all() and (np.abs(w0) < 0.05).any()       # both branches occur, and w passes 0
    run, w = np.zeros(Tn, int), sc.weights(2.0, 6)
    plain = sc.smooth(x, np.zeros((Tn, 10)), np.zeros((Tn, 3)), run, w)
    real = sc.unit_quat
    try:
        sc.unit_quat = lambda R, dtype=np.float64: real(R, dtype) * np.where(np.arange(Tn) % 2 == 1, -1.0, 1.0)[:, None, None]
        flipped = sc.smooth(x, np.zeros((Tn, 10)), np.zeros((Tn, 3)), run, w)
        jit_flipped = sc.jitter(x, run)
    finally:
        sc.unit_quat = real
    assert sc.dist_rot(flipped[0], plain[0]) <= 1e-15 and sc.dist_deg(flipped[3], plain[3]) <= 1e-15
    assert sc.dist_deg(jit_flipped, sc.jitter(x, run)) <= 1e-15
    inner = slice(6, Tn - 6)
    assert sc.dist_rot(plain[0][inner], x[inner]) <= 1e-14                          # and across w = 0 the constant velocity survives


def test_windows_truncate_at_run_ends():
    x = sc.trajectories(2, lengths=(7, 5)).astype(np.float64)
    run = np.repeat([0, 1], [7, 5])
    (both, b_both, _, _), betas, cam = _smooth64(x, run, 6)
    alone = sc.smooth(x[:7], betas[:7], cam[:7], run[:7], sc.weights(2.0, 6))
    assert np.array_equal(both[:7], alone[0]) and np.array_equal(b_both[:7], alone[1])
    alone = sc.smooth(x[7:], betas[7:], cam[7:], run[7:], sc.weights(2.0, 6))
    assert np.array_equal(both[7:], alone[0]) and np.array_equal(b_both[7:], alone[1])
    jit = sc.jitter(x, run)
    assert np.isnan(jit[[0, 6, 7, 11]]).all() and np.isfinite(np.delete(jit, [0, 6, 7, 11])).all()
    # a run of length 1 and radius 0: betas and cam to the bit, the 6-D values orthonormalised
    one = sc.smooth(x[:1].astype(F), betas[:1].astype(F), cam[:1].astype(F), run[:1], sc.weights(2.0, 6), F)
    zero = sc.smooth(x.astype(F), betas.astype(F), cam.astype(F), run, sc.weights(2.0, 0), F)
    assert np.array_equal(one[1], betas[:1].astype(F)) and np.array_equal(zero[1], betas.astype(F)) and np.array_equal(zero[2], cam.astype(F))
    R = sc.rot6d(zero[0])
    assert np.abs(R.transpose(0, 1, 3, 2) @ R - np.eye(3)).max() <= 1e-6 and sc.dist_rot(zero[0], x) <= 1e-6


def test_smoothing_strictly_lowers_the_jitter_of_jittered_input():
    x = sc.trajectories(3, lengths=(40,)).astype(np.float64)
    run = np.zeros(40, int)
    before = sc.jitter(x, run)
    (x_out, _, _, delta), _, _ = _smooth64(x, run, 6)
    after = sc.jitter(x_out, run)
    print(f'jitter {np.nanmean(before):.4f} -> {np.nanmean(after):.4f} deg/frame^2, moved {delta.mean():.4f} deg')
    assert np.nanmean(after) < 0.5 * np.nanmean(before) and (after[1:-1] < before[1:-1]).mean() > 0.9 and delta.mean() > 0.1


def test_a_non_finite_row_stays_in_its_windows():
    table, order, run = sc.table_case(4)
    x6d, betas, cam = sc.positions_of(table, order)
    w = sc.weights(2.0, 6)
    clean = sc.smooth(x6d, betas, cam, run, w, F)
    bad = x6d.copy()
    bad[20, 3] = np.nan                                                             # position 20 of the run of 33 (positions 6 .. 38)
    got = sc.smooth(bad, betas, cam, run, w, F)
    hit = np.zeros(sc.M, bool)
    hit[14:27] = True
    assert np.isnan(got[0][hit, 3]).all() and np.array_equal(got[0][~hit], clean[0][~hit]) and np.array_equal(got[1], clean[1])
    assert np.array_equal(np.delete(got[0], 3, 1), np.delete(clean[0], 3, 1))       # the other joints do not see it
    assert np.array_equal(np.isnan(got[3]), hit)


@pytest.mark.parametrize('radius', sc.RADII)
def test_float32_restatement_stays_close_to_float64(radius):
    """the yardsticks the GPU tests scale, on the GPU tests' own table"""
    table, order, run = sc.table_case(4)
    x6d, betas, cam = sc.positions_of(table, order)
    w = sc.weights(2.0, radius)
    a, b = sc.smooth(x6d, betas, cam, run, w, F), sc.smooth(x6d, betas, cam, run, w, np.float64)
    d = (sc.dist_rot(a[0], b[0]), sc.dist(a[1], b[1]), sc.dist(a[2], b[2]), sc.dist_deg(a[3], b[3]), sc.dist_deg(sc.jitter(x6d, run, F), sc.jitter(x6d, run)))
    print(f'radius {radius}: rotation {d[0]:.3e}  betas {d[1]:.3e}  cam {d[2]:.3e}  delta {d[3]:.3e} rad  jitter {d[4]:.3e} rad')
    assert max(d) <= 5e-6 and min(d[0], d[4]) > 0
    if radius == 0:
        assert d[1] == 0 and d[2] == 0


# ---- 3. the C ABI ----
def test_smooth_symbols_declared_exported_and_in_the_table():
    hdr = open(os.path.join(ROOT, 'include', 'jrr.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    lib_mod, refined, engine = _mod('_lib'), _mod('refined'), _mod('engine')
    _mod('build').build(verbose=False)
    lib = lib_mod.load()
    for name in ('jrr_pose_smooth', 'jrr_pose_jitter'):
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in lib_mod.SIGNATURES and hasattr(lib, name), name
        assert re.search(r'\|[^|\n]*`' + name + r'`[^|\n]*\|', doc), name
    assert 'smooth.hip' in _mod('build').SOURCES
    consts = {k: int(v) for k, v in re.findall(r'\b(JRR_SMOOTH_[A-Z0-9_]+) = (\d+)\b(?! <<)', hdr)}
    assert consts == {'JRR_SMOOTH_MAX_RADIUS': refined.SMOOTH_MAX_RADIUS, 'JRR_SMOOTH_TILE': 32, 'JRR_SMOOTH_STATUS_INDEX': 1,
                      'JRR_SMOOTH_STATUS_MARKER': 2}
    assert refined.SMOOTH_MAX_RADIUS == engine.SMOOTH_MAX_RADIUS == 16 and set(refined.SMOOTH_STATUS_BITS) == {1, 2}
    # argument errors come back as a status, nothing is launched (the pointers are never read)
    import ctypes
    p, p16 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 16)
    names = ('t', 'n', 'o', 'r', 'm', 'w', 'rad', 'b', 'c', 'x', 'be', 'ca', 'd', 's', 'st')
    base = dict(t=p, n=64, o=p, r=p, m=40, w=p, rad=6, b=0, c=0, x=p16, be=p, ca=p, d=p, s=p, st=None)
    smooth = lambda **kw: lib.jrr_pose_smooth(*[dict(base, **kw)[k] for k in names])
    assert smooth() == 0 and smooth(b=40) == 0                                     # an empty range launches nothing
    for k in ('t', 'o', 'r', 'w', 'x', 'be', 'ca', 'd', 's'):
        assert smooth(**{k: None}) == -1, k
    assert smooth(rad=17) == -1 and b'radius 17' in lib.jrr_last_error() and smooth(rad=-1) == -1
    assert smooth(b=-1) == -1 and smooth(b=41) == -1 and smooth(c=41) == -1 and smooth(b=30, c=11) == -1
    assert b'position range' in lib.jrr_last_error()
    assert smooth(b=30, c=2147483647) == -1                                         # begin + count is never formed
    assert smooth(n=-1) == -1 and smooth(n=1 << 31) == -1 and smooth(m=-1) == -1
    assert smooth(x=ctypes.c_void_p(4096 + 8)) == -1 and b'16-byte aligned' in lib.jrr_last_error()
    assert smooth(t=ctypes.c_void_p(4096 + 4)) == -1 and b'8-byte aligned' in lib.jrr_last_error()
    jnames = ('t', 'n', 'o', 'r', 'm', 'b', 'c', 'j', 's', 'st')
    jbase = dict(t=p, n=64, o=p, r=p, m=40, b=0, c=0, j=p, s=p, st=None)
    jitter = lambda **kw: lib.jrr_pose_jitter(*[dict(jbase, **kw)[k] for k in jnames])
    assert jitter() == 0
    for k in ('t', 'o', 'r', 'j', 's'):
        assert jitter(**{k: None}) == -1, k
    assert jitter(c=41) == -1 and jitter(b=-1) == -1 and jitter(j=ctypes.c_void_p(4098)) == -1


def test_weights_are_rounded_once_from_float64():
    refined = _mod('refined')
    w = refined.smooth_weights(2.0)
    assert w.dtype == F and w.shape == (7,) and w[0] == 1.0 and np.array_equal(w, sc.weights(2.0, 6))
    assert w[3] == F(np.exp(-9.0 / 8.0)) and (np.diff(w) < 0).all()
    assert refined.smooth_weights(0.2).shape == (2,) and refined.smooth_weights(50.0).shape == (17,)          # ceil(3 sigma), at most 16
    assert refined.smooth_weights(2.0, 0).tolist() == [1.0] and refined.smooth_weights(1.0, 16).shape == (17,)
    for bad in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float('nan')), dict(sigma=2.0, radius=17), dict(sigma=2.0, radius=-1)):
        with pytest.raises(ValueError):
            refined.smooth_weights(**bad)


def test_flags_default_to_off():
    a = _mod('args')
    ns = a.get_args([])
    assert ns.smooth_refined is None and ns.smooth_sigma == 2.0 and ns.smooth_radius is None
    ns = a.get_args(['--smooth_refined', 'dir', '--smooth_sigma', '1.5', '--smooth_radius', '4'])
    assert ns.smooth_refined == 'dir' and ns.smooth_sigma == 1.5 and ns.smooth_radius == 4
    for k, v in a.REFERENCE_FLAGS.items():
        assert getattr(ns, k) == v, k
    saved = a._LazyArgs._ns
    try:
        a._LazyArgs._ns = a.get_args(['--smooth_refined', 'somewhere'])
        with pytest.raises(ValueError, match='--smooth_refined needs --data_root'):
            _mod('refined').smooth_command(log=lambda s: None)
    finally:
        a._LazyArgs._ns = saved


# ---- 4. the files, with the three operators restated on the host ----
def _write_6d_dataset(root, n, seed):
    loc = os.path.join(root, 'precomputed_val')
    os.makedirs(loc)
    g = torch.Generator().manual_seed(seed)
    files = dict(bboxes=torch.tensor([[100., 200., 700., 600.]]).repeat(n, 1), betas=torch.randn(n, 10, generator=g),
                 estimated_translation=torch.randn(n, 3, generator=g), gt_j2d=torch.rand(n, 17, 2, generator=g) * 1000,
                 gt_j3d=torch.randn(n, 17, 3, generator=g) * 300, intrinsics=torch.eye(3).repeat(n, 1, 1),
                 orient=torch.randn(n, 1, 6, generator=g), pose=torch.randn(n, 23, 6, generator=g))
    for k, v in files.items():
        torch.save(v, os.path.join(loc, f'{k}.pt'))
    return files


def _host_operators(monkeypatch):
    """engine.pose_jitter / pose_smooth / pose_export on CPU tensors by the float32 restatement (the GPU tests hold the kernels to it)"""
    engine = _mod('engine')

    def positions(table, order):
        return sc.positions_of(table.numpy(), order.numpy())

    def pose_jitter(table, order, run, status, begin=0, count=None, out=None):
        return T(sc.jitter(positions(table, order)[0], run.numpy(), F))

    def pose_smooth(table, order, run, weights, status, begin=0, count=None, out=None):
        x6d, betas, cam = positions(table, order)
        return tuple(T(np.ascontiguousarray(a)) for a in sc.smooth(x6d, betas, cam, run.numpy(), weights.numpy(), F))

    def pose_export(x6d, betas, cam, index, table, status, extra=None):
        assert (table[index, 229] == 0).all()                                       # the caller cleared the markers of the rows it lists
        table[index] = T(rc.host_rows(x6d.numpy(), betas.numpy(), cam.numpy(), None if extra is None else extra.numpy()))

    for f in (pose_jitter, pose_smooth, pose_export):
        monkeypatch.setattr(engine, f.__name__, f)


def _write_table(directory, seed=4):
    """DIR/refined.npz + meta.json holding sc.table_case (the axis-angle part consistent with the 6-D part); (arrays, order, run)"""
    refined = _mod('refined')
    table, order, run = sc.table_case(seed)
    x6d, betas, cam = sc.positions_of(table, order)
    table[order] = rc.host_rows(x6d, betas, cam, table[order, 230:237])
    t = refined.RefinedTable(sc.N_ROWS, 'cpu')
    t.table.copy_(T(table))
    return t.finish(directory, {'inner_iters': 3, 'data': 'dataset'}), order, run


def _keys_frames(order, run):
    """(keys, frames) per table row that make sequence_runs return exactly (order, run): the row's run as its key, its place as frame"""
    keys, frames = np.full(sc.N_ROWS, 99), np.full(sc.N_ROWS, -1)
    keys[order], frames[order] = run, np.arange(sc.M) * 5
    return keys, frames


def test_smooth_files_round_trip_through_load(tmp_path, monkeypatch):
    refined = _mod('refined')
    _host_operators(monkeypatch)
    out_dir = str(tmp_path / 'ref')
    raw, order, run = _write_table(out_dir)
    raw_bytes = open(os.path.join(out_dir, 'refined.npz'), 'rb').read()
    meta_before = json.load(open(os.path.join(out_dir, 'meta.json')))
    keys, frames = _keys_frames(order, run)
    o, r, f = refined.sequence_runs((keys, frames), raw['has_refined'])
    assert np.array_equal(o, order) and np.array_equal(r, run)
    out = refined.smooth(out_dir, (keys, frames), sigma=2.0, device='cpu',
                         rescore=lambda a, b: ({'mpjpe_eval_mm_raw': a['mpjpe_mm'] + 1}, {'mpjpe_eval_mm_raw_mean': 7.5}))
    assert sorted(os.listdir(out_dir)) == ['meta.json', 'refined.npz', 'refined_smooth.npz']
    assert open(os.path.join(out_dir, 'refined.npz'), 'rb').read() == raw_bytes      # refined.npz itself is not rewritten
    back = refined.load(out_dir, n=sc.N_ROWS, name='refined_smooth.npz')
    meta = back.pop('meta')
    assert set(back) == set(raw) | {'jitter_deg_raw', 'jitter_deg', 'smooth_delta_deg', 'run_id', 'run_len', 'frame', 'mpjpe_eval_mm_raw'}
    assert all(np.array_equal(back[k], out[k], equal_nan=True) for k in back)
    # the records: the restatement's, at their rows; the extras and the unlisted rows as they were
    x6d, betas, cam = sc.positions_of(refined.pack(raw), order)
    want = sc.smooth(x6d, betas, cam, run, sc.weights(2.0, 6), F)
    assert np.array_equal(back['pose6d'][order], want[0]) and np.array_equal(back['shape'][order], want[1]) and np.array_equal(back['cam'][order], want[2])
    assert np.array_equal(back['pose'][order], rc.log_map(rc.rot6d(want[0].reshape(-1, 6), F), F).reshape(sc.M, 72))
    assert np.array_equal(back['has_refined'], raw['has_refined']) and back['has_refined'].sum() == sc.M
    for name in refined.EXTRA_NAMES + ('mpjpe_mm', 'pampjpe_mm'):
        assert np.array_equal(back[name], raw[name], equal_nan=True), name
    rest = np.setdiff1d(np.arange(sc.N_ROWS), order)
    assert not back['pose6d'][rest].any() and np.isnan(back['jitter_deg'][rest]).all() and np.isnan(back['smooth_delta_deg'][rest]).all()
    assert (back['run_id'][rest] == -1).all() and (back['run_len'][rest] == -1).all() and (back['frame'][rest] == -1).all()
    assert np.array_equal(back['run_id'][order], run) and np.array_equal(back['run_len'][order], np.repeat(sc.RUN_LENGTHS, sc.RUN_LENGTHS))
    assert np.array_equal(back['frame'][order], np.arange(sc.M) * 5) and back['frame'].dtype == np.int64 and back['run_id'].dtype == np.int32
    assert np.array_equal(back['smooth_delta_deg'][order], want[3])
    assert np.array_equal(back['jitter_deg_raw'][order], sc.jitter(x6d, run, F), equal_nan=True)
    assert np.array_equal(back['jitter_deg'][order], sc.jitter(want[0], run, F), equal_nan=True)
    assert np.isfinite(back['jitter_deg'][order]).sum() == (3 - 2) + (33 - 2) + (31 - 2)
    s = meta['smooth']
    assert s['sigma'] == 2.0 and s['radius'] == 6 and s['runs'] == 5 and s['positions'] == sc.M and s['mpjpe_eval_mm_raw_mean'] == 7.5
    assert s['run_length_histogram'] == {'1': 1, '2': 1, '3': 1, '31': 1, '33': 1}
    assert s['jitter_deg_mean'] < s['jitter_deg_raw_mean'] and s['smooth_delta_deg_mean'] > 0
    np.testing.assert_allclose(s['jitter_deg_mean'], np.nanmean(back['jitter_deg'].astype(np.float64)), rtol=1e-12)
    assert {k: v for k, v in meta.items() if k != 'smooth'} == meta_before and 'smooth' not in meta_before
    # the plain load still reads refined.npz, and a second smoothing starts from it again
    assert np.array_equal(refined.load(out_dir)['pose6d'], raw['pose6d'])
    again = refined.smooth(out_dir, (keys, frames), sigma=2.0, radius=6, device='cpu')
    assert np.array_equal(again['pose6d'], out['pose6d']) and 'mpjpe_eval_mm_raw' not in again
    # an explicit radius, and nothing listed at all
    r0 = refined.smooth(out_dir, (keys, frames), sigma=2.0, radius=0, device='cpu')
    assert np.array_equal(r0['shape'], raw['shape']) and np.array_equal(r0['cam'], raw['cam']) and r0['meta']['smooth']['radius'] == 0
    assert np.array_equal(np.signbit(r0['shape']), np.signbit(raw['shape']))


def test_init_refined_reads_the_npz_form(tmp_path, monkeypatch):
    refined, batches = _mod('refined'), _mod('batches')
    _host_operators(monkeypatch)
    out_dir = str(tmp_path / 'ref')
    raw, order, run = _write_table(out_dir)
    refined.smooth(out_dir, _keys_frames(order, run), sigma=2.0, device='cpu')
    by_dir, by_file = refined.load_path(out_dir), refined.load_path(os.path.join(out_dir, 'refined_smooth.npz'))
    plain = refined.load_path(os.path.join(out_dir, 'refined.npz'))
    assert np.array_equal(by_dir['pose6d'], raw['pose6d']) and np.array_equal(plain['pose6d'], raw['pose6d'])
    assert 'jitter_deg' in by_file and 'jitter_deg' not in by_dir and not np.array_equal(by_file['pose6d'], raw['pose6d'])
    with pytest.raises(ValueError, match='holds 96 samples, 95 expected'):
        refined.load_path(os.path.join(out_dir, 'refined_smooth.npz'), n=95)
    # the driver's loader starts the listed samples from the smoothed rows
    root = str(tmp_path / 'data')
    os.makedirs(root)
    files = _write_6d_dataset(root, sc.N_ROWS, 1)
    seen = 0
    for full in batches.dataset_batches(root, 40, 0, 'cpu', init_refined=by_file):
        idx = full['index'].numpy()
        has = by_file['has_refined'][idx].astype(bool)
        assert np.array_equal(full['pose6d'].numpy()[has], by_file['pose6d'][idx[has]]) and np.array_equal(full['betas'].numpy()[has], by_file['shape'][idx[has]])
        assert torch.equal(full['betas'][T(~has)], files['betas'][T(idx[~has])])
        seen += int(has.sum())
    assert seen == sc.M
    # optimize.Run.batches resolves the flag through load_path
    src = open(os.path.join(ROOT, PKG_NAME, 'optimize.py')).read()
    assert 'jrefined.load_path(args.init_refined)' in src


def test_command_refuses_a_split_of_another_length(tmp_path, monkeypatch):
    a, refined = _mod('args'), _mod('refined')
    _host_operators(monkeypatch)
    out_dir = str(tmp_path / 'ref')
    _write_table(out_dir)
    root = str(tmp_path / 'data')
    os.makedirs(root)
    _write_6d_dataset(root, sc.N_ROWS - 1, 1)
    saved = a._LazyArgs._ns
    try:
        a._LazyArgs._ns = a.get_args(['--smooth_refined', out_dir, '--data_root', root])
        with pytest.raises(FileNotFoundError, match='images.pkl'):
            refined.smooth_command(log=lambda s: None)
        with open(os.path.join(root, 'precomputed_val', 'images.pkl'), 'wb') as f:
            pickle.dump([_path('Walking', '1', k) for k in range(sc.N_ROWS - 1)], f)
        with pytest.raises(ValueError, match='the table holds 96 samples, the split 95 with 95 frame paths'):
            refined.smooth_command(log=lambda s: None)
    finally:
        a._LazyArgs._ns = saved
