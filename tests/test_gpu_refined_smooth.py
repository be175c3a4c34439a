"""The time-axis filter over the refined-pose table on the GPU (pytest -m gpu): jrr_pose_smooth and jrr_pose_jitter against the float64
evaluation of the host restatement (tests/refined_smooth_cases.py), the properties the header promises, refined.smooth on a table the
driver wrote from a dataset directory with sequence paths, and the `--smooth_refined` command with its re-evaluation.

Bounds: there is no reference implementation, so every comparison is held to `3 x (distance of the restatement's float32 evaluation
from its float64 evaluation on THIS test's inputs) + 1e-7` (refined_smooth_cases.bound), the maximum over all entries; rotations are
compared as matrices, angles in radians.

Shapes: a 96-row table, 70 listed rows in a non-monotone order with the unrefined rows in between, runs of 1, 2, 3, 33 and 31
positions (three workgroups of 32 positions, the last with 6; the long runs and their windows straddle the tiles), radius 0, 1, 6 and
16.  Joints cycle through any angle / within 1e-3 of pi / the exact identity / a sequence whose quaternion passes w = 0.
"""
import importlib
import os
import pickle

import numpy as np
import pytest
import torch

import eval_report_cases as ec
import refined_cases as rc
import refined_smooth_cases as sc
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
F = np.float32
SIGMA = 2.0


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


class Case:
    """the table of refined_smooth_cases.table_case on the device, with what the restatement says about it (computed once, never
    changed)"""

    def __init__(self, seed=4):
        self.table_np, self.order_np, self.run_np = sc.table_case(seed)
        self.x6d, self.betas, self.cam = sc.positions_of(self.table_np, self.order_np)
        self.table, self.order, self.run = T(self.table_np).to(DEV), T(self.order_np).to(DEV), T(self.run_np).to(DEV)
        self.ref = {}

    def yardstick(self, radius, valid=None):
        """(float64 outputs, distances of the float32 outputs from them) of smooth at this radius"""
        key = (radius, None if valid is None else tuple(valid.tolist()))
        if key not in self.ref:
            w = sc.weights(SIGMA, radius)
            r64 = sc.smooth(self.x6d, self.betas, self.cam, self.run_np, w, np.float64, valid)
            r32 = sc.smooth(self.x6d, self.betas, self.cam, self.run_np, w, F, valid)
            self.ref[key] = (r64, _distances(r32, r64))
        return self.ref[key]

    def smooth(self, radius, table=None, order=None, run=None, **kw):
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = _mod('engine').pose_smooth(self.table if table is None else table, self.order if order is None else order,
                                         self.run if run is None else run, T(sc.weights(SIGMA, radius)).to(DEV), status, **kw)
        return [t.cpu().numpy() for t in out], int(status.item())

    def jitter(self, table=None, order=None, run=None, **kw):
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = _mod('engine').pose_jitter(self.table if table is None else table, self.order if order is None else order,
                                         self.run if run is None else run, status, **kw)
        return out.cpu().numpy(), int(status.item())


def _distances(got, want):
    return (sc.dist_rot(got[0], want[0]), sc.dist(got[1], want[1]), sc.dist(got[2], want[2]), sc.dist_deg(got[3], want[3]))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope='module')
def case():
    return Case()


# ---- 1. both kernels against float64 ----
@pytest.mark.parametrize('radius', sc.RADII)
def test_pose_smooth_against_float64(case, radius):
    before = case.table.clone()
    got, status = case.smooth(radius)
    want, d = case.yardstick(radius)
    g = _distances(got, want)
    for name, gv, dv in zip(('rotation', 'betas', 'cam', 'delta rad'), g, d):
        print(f'radius {radius}: {name} {gv:.3e} (yardstick {dv:.3e}, bound {sc.bound(dv):.3e})')
    assert status == 0
    for gv, dv in zip(g, d):
        assert gv <= sc.bound(dv)
    assert torch.equal(_as_int(case.table), _as_int(before))                       # the input table is unchanged byte for byte
    # every output is a rotation's first two columns; the identity joints stay the exact identity
    R = sc.rot6d(got[0])
    assert np.abs(R[..., :2] - got[0].reshape(sc.M, 24, 3, 2)).max() <= 1e-6
    assert np.array_equal(got[0][:, 2::4], np.broadcast_to(F([1, 0, 0, 1, 0, 0]), (sc.M, 6, 6)))
    if radius == 0:                                                               # betas and cam to the bit, the signed zeros included
        assert np.array_equal(_bits(got[1]), _bits(case.betas)) and np.array_equal(_bits(got[2]), _bits(case.cam))
        assert np.signbit(got[1][5, 0]) and np.signbit(got[2][40, 1])
    lone = np.repeat(np.array(sc.RUN_LENGTHS) == 1, sc.RUN_LENGTHS)                # a run of length 1: the same at every radius
    assert np.array_equal(_bits(got[1][lone]), _bits(case.betas[lone])) and np.array_equal(_bits(got[2][lone]), _bits(case.cam[lone]))


def _as_int(t):
    return t.view(torch.int32)


def test_pose_jitter_against_float64(case):
    before = case.table.clone()
    got, status = case.jitter()
    want, j32 = sc.jitter(case.x6d, case.run_np), sc.jitter(case.x6d, case.run_np, F)
    d, g = sc.dist_deg(j32, want), sc.dist_deg(got, want)
    print(f'jitter {g:.3e} rad (yardstick {d:.3e}, bound {sc.bound(d):.3e}); mean {np.nanmean(got):.4f} deg/frame^2')
    assert status == 0 and g <= sc.bound(d)
    assert np.isfinite(got).sum() == 1 + 31 + 29 and np.isnan(got[[0, 1, 2, 3, 5, 6, 38, 39, 69]]).all()
    assert torch.equal(_as_int(case.table), _as_int(before))
    # a constant angular velocity about a fixed axis: zero up to the rounding of the inputs
    x = np.stack([sc.constant_velocity(40, (1, 2, 3), 0.3, 0.07)] * 24, 1).astype(F)
    table = np.zeros((40, sc.ROW), dtype=F)
    table[:, 72:216], table[:, 229] = x.reshape(40, 144), 1.0
    order, run = torch.arange(40, dtype=torch.int32, device=DEV), torch.zeros(40, dtype=torch.int32, device=DEV)
    flat, _ = case.jitter(T(table).to(DEV), order, run)
    d_flat = sc.dist_deg(sc.jitter(x, np.zeros(40, int), F), sc.jitter(x, np.zeros(40, int)))
    print(f'constant velocity: jitter {np.nanmax(flat):.3e} deg; float32 restatement from float64 {d_flat:.3e} rad')
    assert sc.dist_deg(flat, sc.jitter(x, np.zeros(40, int))) <= sc.bound(d_flat)


def test_outputs_stay_inside_their_arrays(case):
    """the entry points on arrays with guard floats on either side, over a position range"""
    lib_mod = _mod('_lib')
    lib, ptr = lib_mod.load(), lib_mod.ptr
    sizes = (sc.M * 144, sc.M * 10, sc.M * 3, sc.M, sc.M)
    bufs = [torch.full((n + 32,), 7.0, device=DEV) for n in sizes]
    outs = [b[16:16 + n] for b, n in zip(bufs, sizes)]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    w = T(sc.weights(SIGMA, 6)).to(DEV)
    begin, count = 3, 41
    lib_mod.check(lib.jrr_pose_smooth(ptr(case.table), sc.N_ROWS, ptr(case.order), ptr(case.run), sc.M, ptr(w), 6, begin, count, ptr(outs[0]),
                                      ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), ptr(status), lib_mod.stream_ptr(case.table.device)), 'smooth')
    lib_mod.check(lib.jrr_pose_jitter(ptr(case.table), sc.N_ROWS, ptr(case.order), ptr(case.run), sc.M, begin, count, ptr(outs[4]), ptr(status),
                                      lib_mod.stream_ptr(case.table.device)), 'jitter')
    torch.cuda.synchronize()
    whole, _ = case.smooth(6)
    whole.append(case.jitter()[0])
    for b, o, full, per in zip(bufs, outs, whole, (144, 10, 3, 1, 1)):
        assert (b[:16] == 7.0).all().item() and (b[-16:] == 7.0).all().item()
        o = o.cpu().numpy().reshape(sc.M, per)
        assert (o[:begin] == 7.0).all() and (o[begin + count:] == 7.0).all()        # rows outside the range are not touched
        assert np.array_equal(_bits(o[begin:begin + count]), _bits(full.reshape(sc.M, per)[begin:begin + count]))
    assert int(status.item()) == 0


# ---- 2. a result depends on its window alone ----
@pytest.mark.parametrize('radius', [6, 16])
def test_a_run_at_another_offset_gives_equal_bits(case, radius):
    """the run of 33 sits at positions 6 .. 38; listed first it sits at 0 .. 32, in other places of other tiles"""
    whole, _ = case.smooth(radius)
    perm = np.concatenate([np.arange(6, 39), np.arange(0, 6), np.arange(39, sc.M)])
    moved, status = case.smooth(radius, order=T(case.order_np[perm]).to(DEV), run=T(case.run_np[perm]).to(DEV))
    assert status == 0
    for a, b in zip(moved, whole):
        assert np.array_equal(_bits(a[:33]), _bits(b[6:39]))
    # ... and alone, as the only run of a shorter list (another M)
    alone, _ = case.smooth(radius, order=T(case.order_np[6:39].copy()).to(DEV), run=T(case.run_np[6:39].copy()).to(DEV))
    for a, b in zip(alone, whole):
        assert np.array_equal(_bits(a), _bits(b[6:39]))
    j_whole, j_moved = case.jitter()[0], case.jitter(order=T(case.order_np[perm]).to(DEV), run=T(case.run_np[perm]).to(DEV))[0]
    assert np.array_equal(_bits(j_moved[:33]), _bits(j_whole[6:39]))


def test_two_launches_over_halves_equal_one(case):
    """each half is given the whole order / run arrays and a position range (35 is not a multiple of the tile)"""
    eng = _mod('engine')
    whole, _ = case.smooth(6)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    w = T(sc.weights(SIGMA, 6)).to(DEV)
    out = eng.pose_smooth(case.table, case.order, case.run, w, status, begin=0, count=35)
    assert torch.isnan(out[3][35:]).all().item() and torch.isfinite(out[3][:35]).all().item()
    out = eng.pose_smooth(case.table, case.order, case.run, w, status, begin=35, count=35, out=out)
    for a, b in zip(out, whole):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b))
    j = eng.pose_jitter(case.table, case.order, case.run, status, begin=0, count=35)
    j = eng.pose_jitter(case.table, case.order, case.run, status, begin=35, out=j)
    assert np.array_equal(_bits(j.cpu().numpy()), _bits(case.jitter()[0])) and int(status.item()) == 0


def test_a_nan_row_changes_exactly_the_positions_whose_window_holds_it(case):
    clean, _ = case.smooth(6)
    j_clean, _ = case.jitter()
    table = case.table.clone()
    table[int(case.order_np[20]), 72 + 3 * 6:72 + 4 * 6] = float('nan')               # joint 3 of position 20 (run of 33: 6 .. 38)
    table[int(case.order_np[50]), 216 + 4] = float('inf')                           # betas[4] of position 50 (run of 31: 39 .. 69)
    got, status = case.smooth(6, table=table)
    assert status == 0
    hit = np.zeros(sc.M, bool)
    hit[14:27] = True
    assert np.isnan(got[0][hit, 3]).all() and np.isnan(got[3][hit]).all()
    assert np.array_equal(_bits(got[0][~hit]), _bits(clean[0][~hit])) and np.array_equal(_bits(got[3][~hit]), _bits(clean[3][~hit]))
    assert np.array_equal(_bits(np.delete(got[0], 3, 1)), _bits(np.delete(clean[0], 3, 1)))
    hit_b = np.zeros(sc.M, bool)
    hit_b[44:57] = True
    assert np.isinf(got[1][hit_b, 4]).all() and np.array_equal(_bits(got[1][~hit_b]), _bits(clean[1][~hit_b]))
    assert np.array_equal(_bits(np.delete(got[1], 4, 1)), _bits(np.delete(clean[1], 4, 1))) and np.array_equal(_bits(got[2]), _bits(clean[2]))
    j, _ = case.jitter(table=table)
    assert np.isnan(j[19:22]).all() and np.array_equal(_bits(np.delete(j, [19, 20, 21])), _bits(np.delete(j_clean, [19, 20, 21])))


# ---- 3. the status word ----
def _skipped_position_checks(case, got, j, skipped):
    """a skipped position: NaN outputs, nobody's neighbour; everything else as the restatement has it, untouched outside its windows"""
    valid = np.ones(sc.M, bool)
    valid[skipped] = False
    want, d = case.yardstick(6, valid)
    g = _distances(got, want)
    print('skipped', skipped, ' '.join(f'{gv:.3e} ({sc.bound(dv):.3e})' for gv, dv in zip(g, d)))
    for gv, dv in zip(g, d):
        assert gv <= sc.bound(dv)
    for a in got:
        assert np.isnan(a[skipped]).all()
    clean, _ = case.smooth(6)
    far = np.ones(sc.M, bool)
    for p in skipped:
        far[max(0, p - 6):p + 7] = False
    for a, b in zip(got, clean):
        assert np.array_equal(_bits(a[far]), _bits(b[far]))
    jw = sc.jitter(case.x6d, case.run_np, np.float64, valid)
    dj = sc.dist_deg(sc.jitter(case.x6d, case.run_np, F, valid), jw)
    assert sc.dist_deg(j, jw) <= sc.bound(dj)


def test_status_bit_0_for_an_index_outside_the_table(case):
    order = case.order_np.copy()
    order[20], order[60] = sc.N_ROWS, -1
    d_order = T(order).to(DEV)
    got, status = case.smooth(6, order=d_order)
    j, status_j = case.jitter(order=d_order)
    assert status == 1 and status_j == 1
    _skipped_position_checks(case, got, j, [20, 60])


def test_status_bit_1_for_a_listed_row_without_marker(case):
    table = case.table.clone()
    table[int(case.order_np[45]), 229] = 0.0
    got, status = case.smooth(6, table=table)
    j, status_j = case.jitter(table=table)
    assert status == 2 and status_j == 2
    _skipped_position_checks(case, got, j, [45])
    table[int(case.order_np[10]), 229] = float('nan')                               # a marker that is not 1.0f, whatever else it is
    order = case.order_np.copy()
    order[0] = 1 << 20
    assert case.smooth(6, table=table, order=T(order).to(DEV))[1] == 3


# ---- 4. through the driver's files ----
def _sequence_dataset(root, smpl_model_np, j_h36m_np, n=40):
    """40 samples of two cameras interleaved in file order: camera 1 with frames 5, 10, ... (one missing), camera 2 with the rest; a
    stray path without imageSequence.  The start poses move slowly along each sequence."""
    sm = _mod('smpl_model')
    rng = np.random.RandomState(3)
    full = sm.synthetic_batch(smpl_model_np, j_h36m_np, n, seed=0)
    cam_of = np.arange(n) % 2
    frame = np.where(cam_of == 0, 5 * (np.arange(n) // 2 + 1), 5 * (np.arange(n) // 2 + 1))
    frame[cam_of == 0] += np.where(np.arange(n // 2) >= 12, 5, 0)                   # camera 1 skips frame 65
    paths = [f'/data/h36m/S9/Walking 1/imageSequence/{c + 1}/img_{f:06d}.jpg' for c, f in zip(cam_of, frame)]
    paths[39] = '/data/elsewhere/000001.jpg'
    base = rng.normal(0, 0.3, size=(2, 24, 3))
    aa = (base[cam_of] + 0.02 * (np.arange(n) // 2)[:, None, None] + rng.normal(0, 0.03, size=(n, 24, 3))).astype(F)
    d = os.path.join(root, 'precomputed_val')
    os.makedirs(d)
    tensors = {'bboxes': torch.tensor([[100., 200., 700., 800.]]).repeat(n, 1), 'betas': T(full['betas']),
               'estimated_translation': T(full['cam']), 'gt_j2d': torch.rand(n, 17, 2) * 1000, 'gt_j3d': T(full['gt_j3d']),
               'intrinsics': torch.eye(3).repeat(n, 1, 1), 'orient': T(aa[:, 0]), 'pose': T(aa[:, 1:].reshape(n, 69))}
    for k, v in tensors.items():
        torch.save(v, os.path.join(d, f'{k}.pt'))
    with open(os.path.join(d, 'images.pkl'), 'wb') as f:
        pickle.dump(paths, f)
    return paths, full


def _with_args(flags, fn):
    argsmod = _mod('args')
    saved = argsmod._LazyArgs._ns
    argsmod._LazyArgs._ns = argsmod.get_args(flags + ['--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent'])
    try:
        torch.manual_seed(0)
        return fn()
    finally:
        argsmod._LazyArgs._ns = saved


@pytest.fixture(scope='module')
def driver_table(tmp_path_factory, smpl_model_np, j_h36m_np):
    """a table the driver wrote from the 40-sample dataset directory (batches of 24: a shuffled loader, a ragged second batch)"""
    root = str(tmp_path_factory.mktemp('smooth_data'))
    paths, full = _sequence_dataset(root, smpl_model_np, j_h36m_np)
    out_dir = os.path.join(root, 'refined')
    flags = ['--batch_size', '24', '--inner_iters', '2', '--device', DEV, '--synthetic', '--data_root', root]
    _with_args(flags + ['--save_refined', out_dir], lambda: _mod('optimize').optimize_pose_refiner(log=lambda r: None))
    return root, out_dir, paths, full, flags


def _check_smoothed_files(out_dir, paths, out, radius):
    refined, eng = _mod('refined'), _mod('engine')
    raw = refined.load(out_dir, n=40)
    assert raw['has_refined'].all()
    order, run, frame = refined.sequence_runs(paths, raw['has_refined'])
    assert np.bincount(run).tolist() == [12, 8, 19, 1] and order[-1] == 39 and sorted(order.tolist()) == list(range(40))
    back = refined.load(out_dir, n=40, name='refined_smooth.npz')
    for k in ('pose', 'pose6d', 'shape', 'cam', 'jitter_deg', 'jitter_deg_raw', 'smooth_delta_deg', 'run_id', 'run_len', 'frame'):
        assert np.array_equal(back[k], out[k], equal_nan=True), k
    x6d, betas, cam = raw['pose6d'][order], raw['shape'][order], raw['cam'][order]
    w = sc.weights(SIGMA, radius)
    want, r32 = sc.smooth(x6d, betas, cam, run, w), sc.smooth(x6d, betas, cam, run, w, F)
    d = _distances(r32, want)
    g = _distances((back['pose6d'][order], back['shape'][order], back['cam'][order], back['smooth_delta_deg'][order]), want)
    print('files:', ' '.join(f'{gv:.3e} ({sc.bound(dv):.3e})' for gv, dv in zip(g, d)))
    for gv, dv in zip(g, d):
        assert gv <= sc.bound(dv)
    jw = sc.jitter(x6d, run)
    assert sc.dist_deg(back['jitter_deg_raw'][order], jw) <= sc.bound(sc.dist_deg(sc.jitter(x6d, run, F), jw))
    js = sc.jitter(back['pose6d'][order], run)
    assert sc.dist_deg(back['jitter_deg'][order], js) <= sc.bound(sc.dist_deg(sc.jitter(back['pose6d'][order], run, F), js))
    # the smoothed `pose` is the log map of the smoothed `pose6d`: through batch_rodrigues it gives those matrices
    R = eng.rot6d_forward(T(back['pose6d']).to(DEV).reshape(-1, 6))
    d_rt = rc.yardsticks(R.cpu().numpy())[3]
    g_rt = float((eng.rodrigues_forward(T(back['pose']).to(DEV).reshape(-1, 3)) - R).abs().max().item())
    print(f'pose -> R against rot6d_forward(pose6d): {g_rt:.3e} (bound {rc.bound(d_rt):.3e})')
    assert g_rt <= rc.bound(d_rt)
    for name in refined.EXTRA_NAMES + ('mpjpe_mm', 'pampjpe_mm', 'has_refined'):
        assert np.array_equal(back[name], raw[name], equal_nan=True), name
    assert np.array_equal(back['run_id'][order], run) and np.array_equal(back['frame'][order], frame) and back['frame'][39] == -1
    s = back['meta']['smooth']
    assert s['runs'] == 4 and s['radius'] == radius and s['run_length_histogram'] == {'1': 1, '8': 1, '12': 1, '19': 1}
    assert s['jitter_deg_mean'] < s['jitter_deg_raw_mean']
    print(f"jitter {s['jitter_deg_raw_mean']:.4f} -> {s['jitter_deg_mean']:.4f} deg/frame^2, moved {s['smooth_delta_deg_mean']:.4f} deg")
    return raw, back


def test_refined_smooth_on_a_table_the_driver_wrote(driver_table):
    root, out_dir, paths, full, flags = driver_table
    refined = _mod('refined')
    raw_bytes = open(os.path.join(out_dir, 'refined.npz'), 'rb').read()
    out = refined.smooth(out_dir, paths, sigma=SIGMA, radius=3, device=DEV)
    assert open(os.path.join(out_dir, 'refined.npz'), 'rb').read() == raw_bytes
    raw, back = _check_smoothed_files(out_dir, paths, out, 3)
    # the smoothed file feeds a run: it starts from those bits
    again = _with_args(flags[:2] + ['--inner_iters', '0'] + flags[4:] + ['--init_refined', os.path.join(out_dir, 'refined_smooth.npz')],
                       lambda: _mod('optimize').optimize_pose_refiner(log=lambda r: None))
    idx = again['index'].numpy()
    assert np.array_equal(again['x6d'].cpu().numpy(), back['pose6d'][idx]) and np.array_equal(again['betas'].cpu().numpy(), back['shape'][idx])


def test_the_smooth_refined_command_with_its_re_evaluation(driver_table, capsys):
    root, out_dir, paths, full, flags = driver_table
    refined, eng, utils = _mod('refined'), _mod('engine'), _mod('utils')
    lines = []
    out = _with_args(['--smooth_refined', out_dir, '--data_root', root, '--synthetic', '--device', DEV, '--batch_size', '24'],
                     lambda: refined.smooth_command(log=lines.append))
    raw, back = _check_smoothed_files(out_dir, paths, out, 6)                       # sigma 2 -> radius min(16, ceil(6))
    assert len(lines) == 1 and lines[0].startswith('smoothed 40 poses in 4 runs (sigma 2, radius 6): jitter ') and 'MPJPE' in lines[0]
    s = back['meta']['smooth']
    names = ('mpjpe_eval_mm_raw', 'pampjpe_eval_mm_raw', 'mpjpe_eval_mm_smooth', 'pampjpe_eval_mm_smooth')
    for name in names:
        assert back[name].shape == (40,) and np.isfinite(back[name]).all() and back[name].dtype == F
        np.testing.assert_allclose(s[name + '_mean'], back[name].astype(np.float64).mean(), rtol=1e-12)
        assert f'{s[name + "_mean"]:.4f}' in lines[0]
    print(lines[0])
    # the same numbers from the operators themselves on the same joints: the initial regressor, the driver's body, the command's chunks
    # (rows 0 .. 23 and 24 .. 39).  The plain error is checked against the mean-error operator (jrr_evaluate, another kernel).  The
    # Procrustes error is checked against jrr_evaluate_joints, the operator the command is defined by, and BOTH operators' per-pose
    # means are held to the float64 reference on those same joints, within 3 x (the reference's own float32 distance from float64
    # there) + 1e-7 m: these poses are unrelated to their targets, which is where the K^T K eigen-decomposition the kernels once
    # used came apart between its two compiled instances.
    from importlib import import_module
    smpl = import_module(f'{PKG_NAME}.smpl').SMPL('/nonexistent', batch_size=1, allow_synthetic=True).to(torch.device(DEV))
    J = T(_mod('smpl_model').default_h36m_regressor('/nonexistent', allow_default=True)).float().to(DEV)
    gt = utils.move_pelvis(T(full['gt_j3d']).to(DEV).float())

    def rescored(arrays):
        out = []
        del host[:]
        for lo, hi in ((0, 24), (24, 40)):
            e = eng.RefineEngine(smpl.device_model, hi - lo)
            e.set_j_regressor(J, utils.find_j_reg_mask(J))
            joints = e.find_joints_forward(T(arrays['shape'][lo:hi]).to(DEV), x6d=T(arrays['pose6d'][lo:hi]).to(DEV))
            g = gt[lo:hi].contiguous()
            err_j, err_pa_j = eng.evaluate_joints(joints, g)
            means = eng.evaluate(joints, g)
            out.append(torch.stack(means + (err_j.mean(1), err_pa_j.mean(1))).cpu().numpy() * 1000)
            host.append((joints.cpu().numpy(), g.cpu().numpy(), means[1].cpu().numpy(), err_pa_j.cpu().numpy()))
        return np.concatenate(out, 1)
    host = []                                           # per chunk: joints, targets (mm), jrr_evaluate's PA means, the (n,17) PA distances
    for arrays, (a, b) in ((raw, names[:2]), (back, names[2:])):
        err, err_pa, err_joints, err_pa_joints = rescored(arrays)
        joints_h, gt_h = np.concatenate([h[0] for h in host]), np.concatenate([h[1] for h in host])
        pa64, pa32 = ec.evaluate_joints(joints_h, gt_h, torch.float64)[2], ec.evaluate_joints(joints_h, gt_h, torch.float32)[2]
        d = np.abs(pa32 - pa64).max()
        g_mean = np.abs(np.concatenate([h[2] for h in host]).astype(np.float64) - pa64.mean(1)).max()
        g_joints = np.abs(np.concatenate([h[3] for h in host]).astype(np.float64).mean(1) - pa64.mean(1)).max()
        print(f'{b}: per-pose PA means against float64: jrr_evaluate {g_mean:.3e} m, jrr_evaluate_joints {g_joints:.3e} m '
              f'(reference {d:.3e}, bound {ec.bound(d):.3e})')
        assert g_mean <= ec.bound(d) and g_joints <= ec.bound(d)
        print(f'{a}: {np.abs(back[a] / err - 1).max():.3e} against jrr_evaluate, {np.abs(back[a] / err_joints - 1).max():.3e} against '
              f'jrr_evaluate_joints;  {b}: {np.abs(back[b] / err_pa - 1).max():.3e}, {np.abs(back[b] / err_pa_joints - 1).max():.3e} (relative)')
        np.testing.assert_allclose(back[a], err, rtol=1e-5)
        np.testing.assert_allclose(back[a], err_joints, rtol=1e-6)
        np.testing.assert_allclose(back[b], err_pa_joints, rtol=1e-6)
    # one process: another rank returns at once
    os.environ['RANK'] = '1'
    try:
        assert _with_args(['--smooth_refined', out_dir, '--data_root', root], lambda: refined.smooth_command(log=lines.append)) is None
    finally:
        del os.environ['RANK']
    assert len(lines) == 1
