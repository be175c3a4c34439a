"""The prices of all mesh vertices on the GPU (pytest -m gpu): jrr_jfit_price against int64 arithmetic (the layout), against the float64
restatement regressor_solve.price_reference (both modes), its accumulation, repeatability and refusals, against the gradients the
existing passes give at listed vertices, and the `--fit_solve --fit_grow` command as a child process.

Bounds.
  Integers: vertices in [-8, 8], weights multiples of 1/8 that sum to 1, ground truth 1000 * integers, MSE, delta = 0.  q is a multiple
  of 1/8 below 8, r a multiple of 1/8 below 24 (gt / 1000.0 is an exact quotient), every product a v and every sum of them a multiple of
  1/8 far below 2^53: S and sum r.r equal the int64 restatement bit for bit in any order of summation.
  Real inputs, per element of S.  S[i][u] = sum over s, c of a v, the device's a in place of the exact one.
    (1) The sum: the products enter the matrix instruction exactly (fused), a term passes through at most 3 rpc + nc + 1 additions (its
        chunk's k groups of one accumulator, the chunks in the finish, the add of `accumulate`), and a carries the relative roundings of
        its last steps (three squares and two adds, a square root and a division in NORM mode: at most 5).  3 rpc + nc + 6 <= 3 batch + 8
        for every batch (rpc = 8 and nc = ceil(batch / 8) up to batch 304; one chunk of the batch itself below 9), so this part is at
        most (3 batch + 8) 2^-53 sum |a| |v|.
    (2) The residual: r_c = q_i,c - q_0,c - gt / 1000 with q a sum of cnt terms in list order, one rounding each (fused), two
        subtractions and one division: |dr_c| <= (cnt_i + cnt_0 + 8) 2^-53 T_c, T_c the sum of the magnitudes of the terms of r_c.  MSE:
        da = dr.  NORM: a = r / rho, d rho <= |r . dr| / rho <= |dr|_2, so |da_c| <= (|dr_c| + |dr|_2) / rho: T_c is replaced by
        (T_c + |T|_2) / rho -- at least the 2 T_c / rho of a single axis, which forgets that rho moves with all three.
    Together  |S - exact| <= 2^-53 [ (3 batch + 8) sum |a| |v| + (cnt_i + cnt_0 + 8) sum T' |v| ]   (jprice_cases.price_bound).
    The scalars: sum r.r within 2^-53 [(batch + 8) sum r.r + 2 (K + 8) sum |r_c| T_c]; sum rho and sum |r| (Lipschitz 1 in r) within
    2^-53 [(batch + 8) their value + (K + 8) sum |T|_2].
    The float64 restatement is itself a rounded sum; tests/test_regressor_grow.py checks on the CPU that summed in two different orders
    it moves by under 5 % of this bound on these inputs (measured: 0.7 %).
  An accumulated sequence (64 then 66 meshes): the two complete sums within their own bounds and one more addition -- below the bound of
  the 130 meshes at once.
  Against the existing passes: the bound above for the prices plus the same bound for jrr_jfit_norm_moments' b_i (the same sum of
  3 count products of a rounded residual), respectively 2 c (3 n + W + 8) 2^-53 (|P|^T |P| |U|) for the gradient from jrr_jfit_moments'
  M (section 3k: |M - exact| <= 3 count 2^-53 sum |a| |b|, then W products on the host).

Shapes.  6890 vertices are fixed by the kernel (431 tiles, the last with 10 live columns; 14 tile blocks, the last with 15 tiles).
Batches 1, 3, 4, 5 (one partial k group, one full, one and a quarter), 64 (8 chunks of 8) and 130 (17 chunks, the last of 2 samples)."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import jprice_cases as C
from conftest import PKG_NAME, ROOT

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
NJ, NV = 17, 6890
ND = 16 * NV + 64
PAD = 4096
SENTINEL = -7.25
DELTA = 1e-5


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _price(verts, gt, cands, x, mode, delta, out=None, accumulate=False):
    return _mod('engine').price_vertices(T(verts).to(DEV), T(gt).to(DEV), cands, None, x, mode, delta, out=out, accumulate=accumulate)


def _framed():
    """an output inside a larger buffer of sentinels: (buffer, the view the pass writes)"""
    buf = torch.full((ND + 2 * PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    return buf, buf[PAD:PAD + ND]


def _frame_untouched(buf):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + ND:] == SENTINEL).all())


# ---- 6. exact integers: the layout, the last partial tile, the partial k group ----
@pytest.mark.parametrize('empty_pelvis', [False, True])
@pytest.mark.parametrize('batch', [1, 3, 4, 5, 64, 130])
def test_integers_are_exact(batch, empty_pelvis):
    rs = _mod('regressor_solve')
    verts, gt = C.integer_meshes(batch)
    cands, x = C.integer_lists(empty_pelvis)
    assert cands[16].size == 128 and cands[5].size == 0 and set(C.EDGE_VERTICES) <= set(cands[16].tolist())
    want = C.integer_reference(verts, gt, cands, x)
    buf, out = _framed()
    got = _price(verts, gt, cands, x, rs.PRICE_MSE, 0.0, out=out).cpu().numpy()
    assert _frame_untouched(buf)
    S, tail = C.split_out(got)
    Sw, tw = C.split_out(want)
    assert np.array_equal(S.view(np.uint64), Sw.view(np.uint64)), (batch, int((S != Sw).sum()))
    assert np.array_equal(tail[:, [0, 3]], tw[:, [0, 3]])
    assert not S[4].any() and not tail[4].any()                     # row 5 is empty: zeros everywhere
    ref = C.split_out(rs.price_reference(verts, gt, cands, x, rs.PRICE_MSE, 0.0))[1]
    np.testing.assert_allclose(tail[:, 1:3], ref[:, 1:3], rtol=1e-13)            # delta = 0: sum rho = sum |r|
    assert np.array_equal(tail[:, 1], tail[:, 2])


# ---- 7. real inputs against the restatement ----
def _within(got, verts, gt, cands, x, mode, delta, factor_batch=None):
    rs = _mod('regressor_solve')
    want = rs.price_reference(verts, gt, cands, x, mode, delta)
    bS, bs = C.price_bound(verts, gt, cands, x, mode, delta, factor_batch)
    S, tail = C.split_out(got)
    Sw, tw = C.split_out(want)
    err = np.abs(S - Sw)
    live = bS > 0
    share = float((err[live] / bS[live]).max())
    share_s = float((np.abs(tail[:, :3] - tw[:, :3]) / np.maximum(bs, 1e-300)).max())
    print(f'batch {verts.shape[0]} mode {mode}: worst share of the bound S {share:.4f}, scalars {share_s:.4f}; S up to {np.abs(Sw).max():.3e}, '
          f'largest distance {err.max():.3e}')
    assert (err <= bS).all() and not err[~live].any()
    assert (np.abs(tail[:, :3] - tw[:, :3]) <= bs).all() and np.array_equal(tail[:, 3], tw[:, 3])
    return share


@pytest.mark.parametrize('empty_pelvis', [False, True])
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('batch', [5, 130])
def test_real_inputs_against_the_restatement(batch, mode, empty_pelvis):
    verts, gt, cands, x = C.float_case(batch, empty_pelvis)
    buf, out = _framed()
    got = _price(verts, gt, cands, x, mode, DELTA if mode else 0.0, out=out).cpu().numpy()
    assert _frame_untouched(buf)
    _within(got, verts, gt, cands, x, mode, DELTA if mode else 0.0)


def test_zero_residual_in_norm_mode():
    """ground truth on the regressed joints: a = 0 / delta = 0 exactly, S = 0, sum rho = batch delta (delta a power of two)"""
    rs = _mod('regressor_solve')
    batch, delta = 5, 2.0 ** -10
    verts, _ = C.integer_meshes(batch)
    cands, x = C.integer_lists(False)
    V = verts.astype(np.float64)
    q = np.stack([np.einsum('e,nec->nc', x[i], V[:, cands[i]]) if cands[i].size else np.zeros((batch, 3)) for i in range(NJ)], 1)
    gt = (1000.0 * (q - q[:, :1])).astype(np.float32)              # multiples of 125: exact in fp32, and gt / 1000.0 is exact
    S, tail = C.split_out(_price(verts, gt, cands, x, rs.PRICE_NORM, delta).cpu().numpy())
    assert not S.any()
    on = np.array([cands[i].size > 0 for i in range(1, NJ)])
    assert np.array_equal(tail[on], np.tile([0.0, batch * delta, 0.0, float(batch)], (int(on.sum()), 1))) and not tail[~on].any()


# ---- 8. accumulation ----
def test_accumulation():
    rs = _mod('regressor_solve')
    cands, x = C.integer_lists(False)
    verts, gt = C.integer_meshes(130)
    buf, out = _framed()
    out.fill_(float('nan'))                                         # accumulate = 0 overwrites whatever the output held
    _price(verts[:64], gt[:64], cands, x, 0, 0.0, out=out)
    _price(verts[64:], gt[64:], cands, x, 0, 0.0, out=out, accumulate=True)
    assert _frame_untouched(buf)
    one = _price(verts, gt, cands, x, 0, 0.0).cpu().numpy()
    S, tail = C.split_out(out.cpu().numpy())
    S1, t1 = C.split_out(one)
    assert np.array_equal(S.view(np.uint64), S1.view(np.uint64)) and np.array_equal(tail[:, [0, 3]], t1[:, [0, 3]])
    for mode in (0, 1):
        verts, gt, cands, x = C.float_case(130, False)
        d = DELTA if mode else 0.0
        out = torch.full((ND,), float('nan'), dtype=torch.float64, device=DEV)
        _price(verts[:64], gt[:64], cands, x, mode, d, out=out)
        _price(verts[64:], gt[64:], cands, x, mode, d, out=out, accumulate=True)
        _within(out.cpu().numpy(), verts, gt, cands, x, mode, d)


# ---- 9. repeatability ----
def test_two_identical_sequences_give_the_same_bits():
    verts, gt, cands, x = C.float_case(130, False)
    runs = []
    for _ in range(2):
        out = _price(verts[:64], gt[:64], cands, x, 1, DELTA)
        _price(verts[64:], gt[64:], cands, x, 1, DELTA, out=out, accumulate=True)
        runs.append(out.cpu().numpy().view(np.uint64))
    assert np.array_equal(runs[0], runs[1])


# ---- 10. refusals ----
def test_refusals():
    lib, eng = _mod('_lib').load(), _mod('engine')
    B = 3
    verts = torch.zeros(B, NV, 3, device=DEV)
    gt = torch.zeros(B, NJ, 3, device=DEV)
    need = ctypes.c_size_t(1)
    assert lib.jrr_jfit_price_bytes(0, ctypes.byref(need)) == 0 and need.value == 0
    assert lib.jrr_jfit_price_bytes(B, ctypes.byref(need)) == ND * 8 and need.value > 0
    scratch = torch.zeros(need.value // 8 + 1, dtype=torch.float64, device=DEV)
    out = torch.full((ND + 1,), SENTINEL, dtype=torch.float64, device=DEV)
    vtx = np.zeros((NJ, 128), dtype=np.int32)
    cnt = np.zeros(NJ, dtype=np.int32)
    x = np.zeros((NJ, 128))
    vtx[1, :2], cnt[1], x[1, :2] = (5, 9), 2, (0.5, 0.5)
    P = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    stream = _mod('_lib').stream_ptr(torch.device(DEV))

    def call(verts_p=verts.data_ptr(), gt_p=gt.data_ptr(), batch=B, v=vtx, c=cnt, w=x, mode=0, delta=0.0, out_p=out.data_ptr(),
             scr_p=scratch.data_ptr(), scr_bytes=need.value, null=None):
        args = [ctypes.c_void_p(verts_p), ctypes.c_void_p(gt_p), batch, P(v, ctypes.c_int32), P(c, ctypes.c_int32), P(w, ctypes.c_double), mode,
                delta, 0, ctypes.c_void_p(out_p), ctypes.c_void_p(scr_p), scr_bytes, stream]
        if null is not None:
            args[null] = None
        return lib.jrr_jfit_price(*args)

    ARG, WORKSPACE = -1, -3
    assert call() == 0
    for k in (0, 1, 3, 4, 5, 9, 10):
        assert call(null=k) == ARG, k
    assert call(verts_p=verts.data_ptr() + 2) == ARG and call(gt_p=gt.data_ptr() + 1) == ARG
    assert call(out_p=out.data_ptr() + 4) == ARG and call(scr_p=scratch.data_ptr() + 4) == ARG
    assert call(batch=0) == ARG and call(batch=-1) == ARG
    for bad in (-1, 129):
        c = cnt.copy()
        c[1] = bad
        assert call(c=c) == ARG
    for bad in (-1, NV):
        v = vtx.copy()
        v[1, 1] = bad
        assert call(v=v) == ARG
    v = vtx.copy()
    v[1, 1] = 5
    assert call(v=v) == ARG                                         # repeated in its row
    v = vtx.copy()
    v[1, 2] = -77                                                   # behind the count: not read
    assert call(v=v) == 0
    assert call(c=np.zeros(NJ, dtype=np.int32)) == ARG             # no row with entries
    assert call(mode=2) == ARG and call(mode=-1) == ARG
    for d in (-1e-9, float('nan'), float('inf')):
        assert call(delta=d) == ARG and call(mode=1, delta=d) == ARG
    assert call(mode=1, delta=0.0) == ARG and call(mode=1, delta=1e-6) == 0
    assert call(scr_bytes=need.value - 1) == WORKSPACE
    assert b'jrr_jfit_price' in lib.jrr_last_error()
    torch.cuda.synchronize()
    assert float(out[ND]) == SENTINEL
    with pytest.raises(_mod('_lib').JrrError):
        eng.price_vertices(verts, gt, [np.array([1, 1])] + [np.zeros(0, dtype=np.int64)] * 16, None, [np.array([0.5, 0.5])] + [np.zeros(0)] * 16,
                           0, 0.0)


# ---- 11. against the existing passes ----
@pytest.fixture(scope='module')
def bodies(smpl_model_np):
    """64 synthetic bodies: (verts (64, 6890, 3), gt (64, 17, 3) pelvis-centred mm, the shipped regressor)"""
    em, sm = _mod('engine'), _mod('smpl_model')
    n = 64
    J_np = sm.default_h36m_regressor('/nonexistent', allow_default=True)
    full = sm.synthetic_batch(smpl_model_np, J_np, n, seed=5)
    x6d, betas = (T(full[k]).to(DEV).contiguous() for k in ('pose6d', 'betas'))
    eng = em.RefineEngine(em.DeviceModel(smpl_model_np, DEV), n, flags=em.FLAG_KEEP_VERTS)
    eng.set_j_regressor(T(J_np))
    _, verts = eng.find_joints_forward(betas, x6d=x6d, return_verts=True)
    verts = verts.cpu().numpy()
    return verts, J_np


def _planted_gt(verts, J_np, faces, seed=3):
    """ground truth (n, 17, 3) mm, NOT centred: joint i on 3 vertices outside one ring of row i's support"""
    rs = _mod('regressor_solve')
    rng = np.random.default_rng(seed)
    ring = rs.ring_candidates(J_np, faces, 1)
    V = verts.astype(np.float64)
    gt = np.zeros((verts.shape[0], NJ, 3))
    for i in range(NJ):
        free = np.setdiff1d(np.arange(NV), ring[i])
        p = rng.choice(free, 3, replace=False)
        w = rng.uniform(0.2, 1.0, 3)
        gt[:, i] = 1000.0 * np.einsum('e,nec->nc', w / w.sum(), V[:, p])
    return gt.astype(np.float32)


def test_prices_at_listed_vertices_are_the_existing_gradients(bodies, smpl_model_np):
    verts, J_np = bodies
    rs, em, utils = _mod('regressor_solve'), _mod('engine'), _mod('utils')
    n = verts.shape[0]
    gt = _planted_gt(verts, J_np, smpl_model_np['faces'])
    gt = gt - gt[:, :1]
    jf = em.RegressorFit(T(J_np).to(DEV), None, n)
    jf.gather(T(verts).to(DEV), T(gt).to(DEV), 0)
    cands = [np.flatnonzero(J_np[i] > 0) for i in range(NJ)]
    assert [c.size for c in cands] == jf.counts
    cols = np.unique(np.concatenate(cands))
    lists = [np.searchsorted(cols, c) for c in cands]
    x = [J_np[i, c].astype(np.float64) / J_np[i, c].astype(np.float64).sum() for i, c in enumerate(cands)]
    worst = {}
    for mode in (0, 1):
        d = DELTA if mode else 0.0
        out = _price(verts, gt, cands, x, mode, d).cpu().numpy()
        g = rs.price_gradients(out, n, cands, mode)
        bS, _ = C.price_bound(verts, gt, cands, x, mode, d)
        c = 2.0 / (n * 51.0) if mode == 0 else 1.0 / (n * 17.0)
        bg = np.zeros((NJ, NV))
        bg[1:] = c * bS
        bg[0] = bg[1:].sum(0)
        if mode == 0:
            M = jf.moments(0, n).cpu().numpy()
            _, grads = rs.loss_from_moments(M, n, lists, x)
            P = np.abs(np.concatenate([verts[:, cols].astype(np.float64), gt.astype(np.float64)], 1)).transpose(0, 2, 1).reshape(3 * n, -1)
            Uabs = np.zeros((cols.size + NJ, NJ))
            for i in range(1, NJ):
                Uabs[lists[i], i] += x[i]
                Uabs[lists[0], i] += x[0]
                Uabs[cols.size + i, i] += 1e-3
            mag = (P.T @ P) @ Uabs                                   # (W, 17)
            other = [c * C.U * (3 * n + cols.size + NJ + 8) * (mag[lists[i], i] if i else mag[lists[0]].sum(1)) for i in range(NJ)]
        else:
            blocks = rs.parse_norm_blocks(jf.norm_moments(x, rs.NORM_INV, d, 0, n).cpu().numpy(), jf.counts)
            grads = rs.norm_gradient(blocks, n, lists)
            other = [bg[i, cands[i]] for i in range(NJ)]
        share = 0.0
        for i in range(NJ):
            err = np.abs(g[i, cands[i]] - grads[i])
            tol = bg[i, cands[i]] + other[i]
            assert (err <= tol).all(), (mode, i, float((err / tol).max()))
            share = max(share, float((err / tol).max()))
        worst[mode] = share
        # the global gap of the device's prices against the host restatement's
        gh = rs.price_gradients(rs.price_reference(verts, gt, cands, x, mode, d), n, cands, mode)
        gap_d, gap_h = rs.global_gap(g, cands, x, None)[0], rs.global_gap(gh, cands, x, None)[0]
        print(f'mode {mode}: worst share of the tolerance at listed vertices {share:.4f}; global gap {gap_d:.9e} (device) {gap_h:.9e} (host)')
        assert abs(gap_d - gap_h) <= 2 * NJ * float(bg.max())
    jf.info()


# ---- 12. the command ----
@pytest.fixture(scope='module')
def command_runs(tmp_path_factory, bodies, smpl_model_np):
    verts, J_np = bodies
    root = str(tmp_path_factory.mktemp('grow_data'))
    vdir = os.path.join(root, 'meshes')
    os.makedirs(vdir)
    np.save(os.path.join(vdir, 'vertices.npy'), verts)
    np.save(os.path.join(vdir, 'gt_j3d.npy'), _planted_gt(verts, J_np, smpl_model_np['faces']))
    common = ['--synthetic', '--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent', '--device', DEV, '--batch_size', '24',
              '--fit_holdout', '0.25', '--fit_from', vdir, '--fit_solve']
    outs = {}
    for loss in ('mse', 'mpjpe'):
        for grow in (None, 6):
            out = os.path.join(root, f'solve_{loss}_{grow}')
            cmd = [sys.executable, os.path.join(ROOT, 'main.py'), '--fit_regressor', out, '--fit_solve_loss', loss] + common
            if grow is not None:
                cmd += ['--fit_grow', str(grow)]
            r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
            with open(os.path.join(out, 'solve.json')) as f:
                outs[loss, grow] = (json.load(f), r.stdout)
    return outs


@pytest.mark.parametrize('loss', ['mse', 'mpjpe'])
def test_the_fit_grow_command(command_runs, loss):
    rs = _mod('regressor_solve')
    plain, _ = command_runs[loss, None]
    doc, stdout = command_runs[loss, 6]
    assert sorted(plain) == sorted(rs.SOLVE_KEYS + (('norm',) if loss == 'mpjpe' else ()))
    assert sorted(doc) == sorted(rs.SOLVE_KEYS + ('grow',) + (('norm',) if loss == 'mpjpe' else ()))
    grow = doc['grow']
    assert sorted(grow) == sorted(rs.GROW_KEYS) and grow['add'] == 8 and grow['max_rounds'] == 6 and grow['eligible'] == 17 * 6890
    rounds = grow['rounds']
    assert 2 <= len(rounds) <= 7 and [r['round'] for r in rounds] == list(range(len(rounds)))
    print(loss, [(r['round'], sum(r['candidates']), r['loss'], r['global_gap'], r['train']['mpjpe_mm']) for r in rounds])
    for r in rounds:
        assert set(rs.GROW_ROUND_KEYS) <= set(r) and r['holdout_loss'] is not None and r['train']['mpjpe_mm'] > 0 and r['holdout']['mpjpe_mm'] > 0
        assert max(r['candidates']) <= 128 and r['gap'] <= r['global_gap'] * (1 + 1e-9) + 1e-15
    for a, b in zip(rounds, rounds[1:]):
        # warm-started at the previous round's weights; the slack is the rounding of a loss formed from the moments of ANOTHER union
        # (section 3k: about 1e-13 of the first loss on bodies of this size)
        assert b['loss'] <= a['loss'] + 1e-9 * rounds[0]['loss']
    assert grow['global_gap'] == rounds[-1]['global_gap'] and grow['global_gap'] < rounds[0]['global_gap']
    # the first round IS the plain command's solve; the grown support does better on the rows it was fitted on
    assert doc['loss']['train_before'] == plain['loss']['train_before']
    if loss == 'mse':
        assert rounds[0]['loss'] == pytest.approx(plain['loss']['train_after'], rel=1e-9)
        assert doc['loss']['train_after'] < plain['loss']['train_after']
    else:
        assert doc['norm']['objective_mm']['final'] < plain['norm']['objective_mm']['final']
    assert doc['final']['train']['mpjpe_mm'] < plain['final']['train']['mpjpe_mm']
    assert doc['support']['candidates'] == rounds[-1]['candidates'] and sum(doc['support']['after']) <= sum(rounds[-1]['candidates'])
    assert 'global gap' in stdout and 'rounds' in stdout and os.path.isfile(doc['checkpoint'])
