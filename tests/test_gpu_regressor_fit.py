"""The regressor fit on the GPU (pytest -m gpu): jrr_jfit_* against the host restatement (tests/jfit_cases.py: torch autograd + torch.optim.Adam
on the dense parameter, after scripts/utils.py:87-114 and scripts/optimize.py:300-312), against jrr_regress_joints and against the
existing J step, the properties include/jrr.h promises, and the `--fit_regressor` command as a child process.

Bounds: gradients are held to 2e-4 of their maximum (the bound of test_gpu_parity.test_j_regressor_grad), losses to rtol 1e-5; everything
else to `jfit_cases.bound(a32, a64) = 3 x (distance of the restatement's float32 run from its float64 run on THIS test's inputs) +
1e-7`, the maximum over all entries.

Shapes: a 150-row table over 400 vertex columns in minibatches of 64, 64 and 22 (and of 1); rows of the regressor with 5, 128 (the
cap), 2, ... 62 entries, row 1 sharing three vertices with the pelvis row, a union of 211 vertices (no multiple of 4), two masked and 34
negative entries that must never move.  The restatement's runs are computed once (jfit_cases.trajectory_case) and shared.
"""
import ctypes
import importlib
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import jfit_cases as jc
import oracle
from conftest import PKG_NAME, ROOT

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'
SPW = 32                      # include/jrr.h JRR_JFIT_SPW: samples per workgroup chunk of the gradient phase


def _mod(name):
    return importlib.import_module(f'{PKG_NAME}.{name}')


def _fit(J, mask, verts, gt_mm, chunk=64):
    """a RegressorFit with the table gathered in chunks (row0 > 0 is exercised)"""
    fit = _mod('engine').RegressorFit(T(J).to(DEV), None if mask is None else T(mask).to(DEV), len(verts))
    for a in range(0, len(verts), chunk):
        fit.gather(T(verts[a:a + chunk]).to(DEV), T(gt_mm[a:a + chunk]).to(DEV), a)
    return fit


def _lists(dense, vtx):
    return jc.to_lists(dense.cpu().numpy() if torch.is_tensor(dense) else dense, vtx)


def _normalised(J, mask):
    return jc.normalise(T(J).double(), None if mask is None else T(mask).double()).numpy()


@pytest.fixture(scope='module')
def case():
    return jc.trajectory_case()


# ---- 1. gather and forward ----
def test_gather_and_forward(case):
    c = case
    fit = _fit(c['J'], c['mask'], c['verts'], c['gt'], chunk=40)
    assert fit.ns == 211 and fit.entries == sum(jc.COUNTS) and fit.counts == list(jc.COUNTS)
    assert fit.info() == (211, 260, 0, list(jc.COUNTS))
    # the cache: the union's vertices, then the ground truth, of every sample
    cols = np.unique(np.concatenate(c['vtx']))
    cache = fit.cache.cpu().numpy()
    assert np.array_equal(cache[:, :3 * 211].reshape(150, 211, 3), c['verts'][:, cols])
    assert np.array_equal(cache[:, 3 * 211:3 * 211 + 51].reshape(150, 17, 3), c['gt'])
    got = fit.joints().cpu().numpy()
    j64 = jc.Restatement(c['J'], c['mask'], dtype=jc.F64).joints(c['verts'])
    j32 = jc.Restatement(c['J'], c['mask'], dtype=jc.F32).joints(c['verts'])
    table = _mod('engine').JointRegressorTable(T(c['J']).to(DEV), T(c['mask']).to(DEV)).regress(T(c['verts']).to(DEV))[0].cpu().numpy()
    b = jc.bound(j32, j64)
    print(f'joints: {jc.dist(got, j64):.3e} from float64, {jc.dist(got, table):.3e} from jrr_regress_joints (bound {b:.3e})')
    assert jc.dist(got, j64) <= b and jc.dist(got, table) <= b
    part = fit.joints(37, 50).cpu().numpy()
    assert np.array_equal(part, got[37:87])


# ---- 2. one step ----
def _one_step(c, fit, batch, first, rows):
    grad = torch.full((17, 128), float('nan'), device=DEV)
    loss = fit.run(batch, first, 1, jc.LR, grad=grad).cpu().numpy()[:1]
    r = jc.Restatement(c['J'], c['mask'], dtype=jc.F64)
    want_loss, want_grad = r.loss_and_grad(c['verts'][rows], c['gt'][rows])
    g, w = grad.cpu().numpy().astype(np.float64), jc.to_lists(want_grad, c['vtx'])
    rel = np.abs(g - w).max() / np.abs(w).max()
    print(f'batch {batch} first {first}: grad {rel:.3e} of its maximum, loss {loss[0]:.8e} against {want_loss:.8e}')
    assert rel < 2e-4
    assert abs(loss[0] - want_loss) <= 1e-5 * abs(want_loss)
    listed = jc.to_lists(np.ones((17, 6890)), c['vtx']) > 0
    assert not g[~listed].any()                                     # zeros behind a row's count
    return r


@pytest.mark.parametrize('batch,first', [(64, 0), (64, 2), (1, 149)])
def test_one_step(case, batch, first):
    c = case
    fit = _fit(c['J'], c['mask'], c['verts'], c['gt'])
    a = first * batch
    _one_step(c, fit, batch, first, slice(a, min(a + batch, 150)))
    assert fit.info()[2] == 1


# ---- 3. the existing J step ----
def test_against_the_existing_j_step(smpl_model_np, j_h36m_np):
    """50 poses of the synthetic body, as test_gpu_parity.test_j_regressor_grad: one fit step over the gathered meshes against
    jrr_j_regressor_grad_support + jrr_j_step_apply_support"""
    em, sm = _mod('engine'), _mod('smpl_model')
    B = 50
    batch = sm.synthetic_batch(smpl_model_np, j_h36m_np, B, seed=31)
    x6d, betas = T(batch['pose6d']).to(DEV).contiguous(), T(batch['betas']).to(DEV).contiguous()
    gt_c = oracle.move_pelvis(T(batch['gt_j3d'])).to(DEV).contiguous()
    eng = em.RefineEngine(em.DeviceModel(smpl_model_np, DEV), B, flags=em.FLAG_KEEP_VERTS)
    J = T(j_h36m_np).to(DEV).clone()
    eng.set_j_regressor(J)
    counts, fits = eng.j_support_info()
    assert fits
    _, verts = eng.find_joints_forward(betas, x6d=x6d, return_verts=True)
    dJs = torch.zeros(17, 128, device=DEV)
    eng.j_regressor_grad_support(x6d, betas, gt_c, dJs)
    Jm, Jv, Js = torch.zeros_like(J), torch.zeros_like(J), torch.zeros(1, dtype=torch.int32, device=DEV)
    eng.j_step_apply_support(J, dJs, Jm, Jv, Js, jc.LR)
    fit = em.RegressorFit(T(j_h36m_np).to(DEV), None, B)
    assert fit.counts == counts and fit.entries == 62
    fit.gather(verts, gt_c, 0)
    grad = torch.zeros(17, 128, device=DEV)
    fit.run(B, 0, 1, jc.LR, grad=grad)
    rel = float((grad - dJs).abs().max() / dJs.abs().max())
    J_fit, m_fit, v_fit = fit.dense()
    vnp, gnp = verts.cpu().numpy(), gt_c.cpu().numpy()
    r32, r64 = jc.Restatement(j_h36m_np, None, dtype=jc.F32), jc.Restatement(j_h36m_np, None, dtype=jc.F64)
    r32.step(vnp, gnp)
    r64.step(vnp, gnp)
    b = jc.bound(r32.raw(), r64.raw())
    d = jc.dist(J_fit.cpu().numpy(), J.cpu().numpy())
    print(f'gradient {rel:.3e} of its maximum; dense J {d:.3e} from the stepped J, {jc.dist(J_fit.cpu().numpy(), r64.raw()):.3e} from float64 (bound {b:.3e})')
    assert rel < 2e-4
    assert d <= b and jc.dist(J_fit.cpu().numpy(), r64.raw()) <= b
    assert torch.equal(J_fit != T(j_h36m_np).to(DEV), J != T(j_h36m_np).to(DEV))       # the same 62 entries moved
    assert torch.equal(m_fit != 0, Jm != 0)


# ---- 4. trajectory ----
def test_trajectory_of_thirty_steps(case):
    """ten epochs of the three minibatches; after every epoch the raw entries, the normalised regressor and the losses against the
    float64 restatement, within `bound` of its float32 run"""
    c = case
    vtx = c['vtx']
    assert c['f64']['closest'] >= 1e-5                              # (test_regressor_fit.py holds the case to all its conditions)
    fit = _fit(c['J'], c['mask'], c['verts'], c['gt'])
    losses = torch.zeros(30, device=DEV)
    worst = [0.0, 0.0]
    for ep in range(10):
        fit.run(jc.BATCH, 0, 3, jc.LR, loss=losses[3 * ep:3 * ep + 3])
        J, _, _ = fit.dense()
        raw = _lists(J, vtx)
        jn = jc.to_lists(_normalised(J.cpu().numpy(), c['mask']), vtx)
        s32, s64 = c['f32']['snaps'][ep], c['f64']['snaps'][ep]
        b_raw, b_jn = jc.bound(s32['raw'], s64['raw']), jc.bound(s32['jn'], s64['jn'])
        d_raw, d_jn = jc.dist(raw, s64['raw']), jc.dist(jn, s64['jn'])
        # the weights the KERNEL stored for its next forward, through jrr_jfit_joints
        b_j, d_j = jc.bound(s32['joints'], s64['joints']), jc.dist(fit.joints().cpu().numpy(), s64['joints'])
        worst = [max(worst[0], d_raw / b_raw), max(worst[1], d_jn / b_jn)]
        print(f'epoch {ep + 1}: raw {d_raw:.3e} (bound {b_raw:.3e}), normalised {d_jn:.3e} (bound {b_jn:.3e}), joints {d_j:.3e} (bound {b_j:.3e})')
        assert d_raw <= b_raw and d_jn <= b_jn and d_j <= b_j
    got = losses.cpu().numpy()
    b_loss = jc.bound(c['f32']['losses'], c['f64']['losses'])
    print(f'losses: {jc.dist(got, c["f64"]["losses"]):.3e} (bound {b_loss:.3e}); worst ratio to the bound: raw {worst[0]:.3f}, normalised {worst[1]:.3f}')
    assert jc.dist(got, c['f64']['losses']) <= b_loss
    assert fit.info()[2] == 30
    # the moments and everything outside the lists
    J, m, v = (t.cpu().numpy() for t in fit.dense())
    m64, v64 = c['f64']['final'].moments()
    m32, v32 = c['f32']['final'].moments()
    assert jc.dist(m, m64) <= jc.bound(m32, m64) and jc.dist(v, v64) <= jc.bound(v32, v64)
    listed = np.zeros(J.shape, dtype=bool)
    for i, vv in enumerate(vtx):
        listed[i, vv] = True
    assert np.array_equal(J[~listed].view(np.uint32), c['J'][~listed].view(np.uint32)) and not m[~listed].any() and not v[~listed].any()


# ---- 5. a minibatch over several workgroups ----
def test_minibatch_over_several_workgroups(case):
    """JRR_JFIT_SPW = 32 samples per workgroup chunk: a minibatch of 86 runs three workgroups (32, 32, 22), the whole table of 150 in
    one minibatch five (the last with 22)"""
    c = case
    assert _mod('engine').JFIT_SPW == SPW and 86 == 2 * SPW + 22 and 150 == 4 * SPW + 22
    fit = _fit(c['J'], c['mask'], c['verts'], c['gt'])
    _one_step(c, fit, 86, 0, slice(0, 86))
    fit = _fit(c['J'], c['mask'], c['verts'], c['gt'])
    _one_step(c, fit, 86, 1, slice(86, 150))
    fit = _fit(c['J'], c['mask'], c['verts'], c['gt'])
    _one_step(c, fit, 150, 0, slice(0, 150))
    # ... and its update
    r32, r64 = jc.Restatement(c['J'], c['mask'], dtype=jc.F32), jc.Restatement(c['J'], c['mask'], dtype=jc.F64)
    r32.step(c['verts'], c['gt'])
    r64.step(c['verts'], c['gt'])
    J = fit.dense()[0].cpu().numpy()
    assert jc.dist(J, r64.raw()) <= jc.bound(r32.raw(), r64.raw())


# ---- 6. properties ----
def test_two_runs_are_bitwise_equal(case):
    c = case
    outs = []
    for _ in range(2):
        fit = _fit(c['J'], c['mask'], c['verts'], c['gt'])
        grad = torch.zeros(17, 128, device=DEV)
        loss = fit.run(150, 0, 1, jc.LR).clone()                     # five workgroups and their slabs
        loss2 = fit.run(jc.BATCH, 0, 3, jc.LR, grad=grad).clone()
        outs.append([t.cpu().numpy().view(np.uint32) for t in (loss, loss2[:3], grad) + fit.dense()])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_a_single_entry_row_keeps_weight_one():
    counts = list(jc.COUNTS)
    counts[7] = 1
    J, mask, cols, vtx = jc.regressor_case(9, counts=tuple(counts))
    verts, gt = jc.table_case(9, J, mask, cols, n_rows=70)
    fit = _fit(J, mask, verts, gt)
    before = fit.joints().cpu().numpy()
    fit.run(32, 0, 3, jc.LR)
    fit.run(32, 0, 3, jc.LR)
    J2 = fit.dense()[0].cpu().numpy()
    jn = _normalised(J2, mask)
    after = fit.joints().cpu().numpy()
    assert jn[7, vtx[7][0]] == 1.0 and (jn[7] != 0).sum() == 1
    assert np.array_equal(after[:, 7], before[:, 7]) and np.array_equal(after[:, 7], verts[:, vtx[7][0]])        # the stored weight is exactly 1
    assert not np.array_equal(after[:, 8], before[:, 8])


def test_argument_checks(case):
    c = case
    em, lib_mod = _mod('engine'), _mod('_lib')
    lib = lib_mod.load()
    fit = _fit(c['J'], c['mask'], c['verts'], c['gt'])
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    loss = torch.zeros(8, device=DEV)
    state0 = fit.state.clone()
    assert lib.jrr_jfit_run(P(fit.state), P(fit.cache), 150, fit.ns, 64, 0, 0, 1e-2, P(loss), None, None) == 0       # n_steps = 0
    assert lib.jrr_jfit_run(P(fit.state), P(fit.cache), 150, fit.ns, 64, 3, 0, 1e-2, P(loss), None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(fit.state, state0) and not loss.any()
    bad = [
        lib.jrr_jfit_run(P(fit.state), P(fit.cache), 150, fit.ns, 64, 0, 4, 1e-2, P(loss), None, None),                 # beyond the last minibatch
        lib.jrr_jfit_run(P(fit.state), P(fit.cache), 150, fit.ns, 64, 2, 2, 1e-2, P(loss), None, None),
        lib.jrr_jfit_run(P(fit.state), P(fit.cache), 150, fit.ns, 64, -1, 1, 1e-2, P(loss), None, None),
        lib.jrr_jfit_run(P(fit.state), P(fit.cache), 150, fit.ns, 0, 0, 1, 1e-2, P(loss), None, None),
        lib.jrr_jfit_run(None, P(fit.cache), 150, fit.ns, 64, 0, 1, 1e-2, P(loss), None, None),
        lib.jrr_jfit_run(P(fit.state), None, 150, fit.ns, 64, 0, 1, 1e-2, P(loss), None, None),
        lib.jrr_jfit_run(P(fit.state), P(fit.cache), 150, fit.ns, 64, 0, 1, 1e-2, None, None, None),
        lib.jrr_jfit_run(P(fit.state), ctypes.c_void_p(fit.cache.data_ptr() + 4), 150, fit.ns, 64, 0, 1, 1e-2, P(loss), None, None),   # misaligned
        lib.jrr_jfit_run(P(fit.state), P(fit.cache), 150, 0, 64, 0, 1, 1e-2, P(loss), None, None),
        lib.jrr_jfit_run(P(fit.state), P(fit.cache), 150, 17 * 128 + 1, 64, 0, 1, 1e-2, P(loss), None, None),
        lib.jrr_jfit_joints(P(fit.state), P(fit.cache), 150, 100, 51, fit.ns, P(loss), None),
        lib.jrr_jfit_joints(P(fit.state), ctypes.c_void_p(fit.cache.data_ptr() + 8), 150, 0, 1, fit.ns, P(loss), None),
        lib.jrr_jfit_joints(P(fit.state), P(fit.cache), 150, 0, 1, fit.ns, None, None),
        lib.jrr_jfit_gather(P(fit.state), None, P(loss), 1, P(fit.cache), 150, 0, fit.ns, None),
        lib.jrr_jfit_gather(P(fit.state), P(fit.cache), P(loss), 2, P(fit.cache), 150, 149, fit.ns, None),
        lib.jrr_jfit_scatter(None, P(loss), None, None, None),
        lib.jrr_jfit_scatter(P(fit.state), None, None, None, None),
        lib.jrr_jfit_prepare(None, None, P(fit.state), fit.state.numel() * 8, None, None),
        lib.jrr_jfit_info(P(fit.state), None, None),
    ]
    assert bad == [-1] * len(bad), bad
    assert b'jrr_jfit_info' in lib.jrr_last_error()
    assert lib.jrr_jfit_prepare(P(fit.J_init), None, P(fit.state), 1024, None, None) == -3
    assert lib.jrr_jfit_cache_bytes(150, fit.ns) == 150 * ((3 * 211 + 51) | 1) * 4 and lib.jrr_jfit_cache_bytes(150, 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(fit.state, state0)                           # no refused call touched the state
    # a row of 129 positive entries and a regressor without a positive entry are refused by prepare; an empty row is not
    J129 = c['J'].copy()
    J129[1, np.setdiff1d(np.arange(6890), c['vtx'][1])[0]] = 0.5
    for J in (J129, -np.abs(c['J'])):
        with pytest.raises(lib_mod.JrrError, match='status -1'):
            em.RegressorFit(T(J).to(DEV), T(c['mask']).to(DEV), 4)
    empty = c['J'].copy()
    empty[3] = 0
    assert em.RegressorFit(T(empty).to(DEV), T(c['mask']).to(DEV), 4).counts[3] == 0
    # without a mask the two masked entries are listed
    assert em.RegressorFit(T(c['J']).to(DEV), None, 4).entries == sum(jc.COUNTS) + 2


def test_an_empty_row_stays_fixed_and_out_of_the_loss(case):
    """a row without a positive entry has no parameters: the steps leave it as it is and its joint out of the loss and the adjoint
    (the mean still divides by count * 17 * 3); every other row moves as the restatement moves it with that joint's error zeroed"""
    c = case
    J = c['J'].copy()
    J[5] = -np.abs(J[5])
    fit = _fit(J, c['mask'], c['verts'], c['gt'])
    assert fit.counts[5] == 0 and fit.entries == sum(jc.COUNTS) - jc.COUNTS[5]
    grad = torch.zeros(17, 128, device=DEV)
    loss = fit.run(jc.BATCH, 0, 3, jc.LR, grad=grad).cpu().numpy()[:3]
    Jd, m, v = (t.cpu().numpy() for t in fit.dense())
    assert np.isfinite(loss).all() and np.isfinite(Jd).all() and np.isfinite(grad.cpu().numpy()).all()
    assert np.array_equal(Jd[5].view(np.uint32), J[5].view(np.uint32)) and not m[5].any() and not v[5].any()
    # the restatement with joint 5 taken out of the error: float64, three steps
    rows = [i for i in range(17) if i != 5]
    outs = {}
    for name, dtype in (('f32', jc.F32), ('f64', jc.F64)):
        r = jc.Restatement(J, c['mask'], dtype=dtype)
        losses = []
        for a, n in jc.schedule(150, jc.BATCH):
            r.opt.zero_grad()
            pred = torch.matmul(jc.normalise(r.J, r.mask)[rows][None], r._t(c['verts'][a:a + n]))
            d = jc.move_pelvis(pred) - r._t(c['gt'][a:a + n])[:, rows] / 1000
            l = (d ** 2).sum() / (n * 51)
            l.backward()
            r.opt.step()
            losses.append(l.item())
        outs[name] = (np.array(losses), r.raw())
    assert np.allclose(loss, outs['f64'][0], rtol=1e-5, atol=0)
    d, b = jc.dist(Jd, outs['f64'][1]), jc.bound(outs['f32'][1], outs['f64'][1])
    print(f'empty row: J {d:.3e} from float64 (bound {b:.3e})')
    assert d <= b
    assert np.isnan(fit.joints(0, 4).cpu().numpy()[:, 5]).all() and np.isfinite(fit.joints(0, 4).cpu().numpy()[:, rows]).all()


def test_a_foreign_ns_is_refused_on_the_device(case):
    """the host cannot know the prepared NS without a read-back: a call with another ns launches, finds the mismatch, writes NaN losses
    and nothing else, and the next jrr_jfit_info reports it"""
    c = case
    lib_mod = _mod('_lib')
    lib = lib_mod.load()
    fit = _fit(c['J'], c['mask'], c['verts'], c['gt'])
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    before = [t.clone() for t in fit.dense()]
    loss = torch.zeros(2, device=DEV)
    assert lib.jrr_jfit_run(P(fit.state), P(fit.cache), 150, fit.ns - 1, 64, 0, 2, 1e-2, P(loss), None, None) == 0
    assert torch.isnan(loss).all()
    after = fit.dense()
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    with pytest.raises(lib_mod.JrrError, match='not the prepared one'):
        fit.info()


# ---- 7. the command ----
N_CMD = 96


def _paths(n):
    """six sequences of 16 frames: two actions x three cameras"""
    return [f'/data/h36m/S9/Act{(i // 16) // 3} 1/imageSequence/{(i // 16) % 3 + 1}/img_{5 * (i % 16 + 1):06d}.jpg' for i in range(n)]


@pytest.fixture(scope='module')
def command_runs(tmp_path_factory, smpl_model_np):
    """a 96-row synthetic --save_refined table with its dataset directory, the same meshes as a vertices directory, and the three child
    processes: the fit from either source, and the evaluation of the second checkpoint"""
    em, sm, refined = _mod('engine'), _mod('smpl_model'), _mod('refined')
    root = str(tmp_path_factory.mktemp('fit_data'))
    J_np = sm.default_h36m_regressor('/nonexistent', allow_default=True)
    full = sm.synthetic_batch(smpl_model_np, J_np, N_CMD, seed=5)
    paths = _paths(N_CMD)
    n = N_CMD
    x6d, betas, cam = (T(full[k]).to(DEV).contiguous() for k in ('pose6d', 'betas', 'cam'))
    eng = em.RefineEngine(em.DeviceModel(smpl_model_np, DEV), n, flags=em.FLAG_KEEP_VERTS)
    eng.set_j_regressor(T(J_np))
    _, verts = eng.find_joints_forward(betas, x6d=x6d, return_verts=True)
    # the ground truth: the joints of ANOTHER regressor on the same support, 2 mm of noise -- something a fit of these meshes can learn
    rng = np.random.RandomState(11)
    other = _normalised(np.where(J_np > 0, J_np * rng.uniform(0.3, 3.0, size=J_np.shape), 0).astype(np.float32), None)
    gt = np.einsum('jv,bvc->bjc', other, verts.cpu().numpy().astype(np.float64)) * 1000.0 + rng.normal(0, 2.0, size=(n, 17, 3))
    gt = gt.astype(np.float32)
    d = os.path.join(root, 'precomputed_val')
    os.makedirs(d)
    tensors = {'bboxes': torch.tensor([[100., 200., 700., 800.]]).repeat(n, 1), 'betas': T(full['betas']),
               'estimated_translation': T(full['cam']), 'gt_j2d': torch.rand(n, 17, 2) * 1000, 'gt_j3d': T(gt),
               'intrinsics': torch.eye(3).repeat(n, 1, 1), 'orient': torch.zeros(n, 3), 'pose': torch.zeros(n, 69)}
    for k, v in tensors.items():
        torch.save(v, os.path.join(d, f'{k}.pt'))
    with open(os.path.join(d, 'images.pkl'), 'wb') as f:
        pickle.dump(paths, f)
    table_dir = os.path.join(root, 'refined')
    table = refined.RefinedTable(n, DEV)
    table.add(torch.arange(n, dtype=torch.int64, device=DEV), x6d, betas, cam)
    table.finish(table_dir, {'data': 'dataset'})
    vdir = os.path.join(root, 'meshes')
    os.makedirs(vdir)
    np.save(os.path.join(vdir, 'vertices.npy'), verts.cpu().numpy())
    np.save(os.path.join(vdir, 'gt_j3d.npy'), gt)
    with open(os.path.join(vdir, 'paths.txt'), 'w') as f:
        f.write('\n'.join(paths) + '\n')
    torch.cuda.synchronize()
    common = ['--synthetic', '--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent', '--device', DEV, '--batch_size', '32']
    outs = {}
    for name, flags in (('table', ['--fit_from', table_dir, '--data_root', root]), ('verts', ['--fit_from', vdir, '--fit_shuffle'])):
        out = os.path.join(root, 'fit_' + name)
        cmd = [sys.executable, os.path.join(ROOT, 'main.py'), '--fit_regressor', out, '--fit_epochs', '5', '--fit_holdout', '0.34'] + flags + common
        r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs[name] = (out, r.stdout)
    rep = os.path.join(root, 'report')
    cmd = [sys.executable, os.path.join(ROOT, 'main.py'), '--eval_vertices', vdir, '--eval_report', rep, '--eval_j_regressor',
           os.path.join(outs['verts'][0], 'retrained_J_Regressor.pt')] + common
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return outs, rep, J_np, verts.cpu().numpy(), gt


@pytest.mark.parametrize('name', ['table', 'verts'])
def test_the_fit_regressor_command(command_runs, name):
    outs, rep, J_np, verts, gt = command_runs
    rf, checkpoint = _mod('regressor_fit'), _mod('checkpoint')
    out, stdout = outs[name]
    assert sorted(os.listdir(out)) == ['fit.json', 'retrained_J_Regressor.pt']
    lines = [l for l in stdout.splitlines() if l.startswith('fitted the regressor on ')]
    assert len(lines) == 1 and 'MPJPE' in lines[0] and lines[0].endswith('retrained_J_Regressor.pt')
    with open(os.path.join(out, 'fit.json')) as f:
        doc = json.load(f)
    assert sorted(doc) == sorted(rf.DOC_KEYS) and doc['source'] == ('refined' if name == 'table' else 'vertices')
    # six sequences, every third held out: 64 rows train in two minibatches of 32, 32 are scored beside them
    assert doc['rows'] == {'train': 64, 'holdout': 32} and doc['steps_per_epoch'] == 2 and len(doc['epochs']) == 5
    loss = [e['loss'] for e in doc['epochs']]
    print(name, 'loss', ' '.join(f'{x:.4e}' for x in loss), 'MPJPE', doc['initial']['train']['mpjpe_mm'], '->', doc['final']['train']['mpjpe_mm'],
          'held out', doc['initial']['holdout']['mpjpe_mm'], '->', doc['final']['holdout']['mpjpe_mm'])
    assert loss[-1] < loss[0] and all(x < loss[0] for x in loss[1:])       # the training loss falls over the 5 epochs
    assert doc['final']['holdout']['mpjpe_mm'] < doc['initial']['holdout']['mpjpe_mm']
    assert doc['final']['train']['mpjpe_mm'] < doc['initial']['train']['mpjpe_mm']
    assert doc['support']['before'] == [int(c) for c in (J_np > 0).sum(1)] and len(doc['support']['after']) == 17
    J = checkpoint.load_j_regressor(os.path.join(out, 'retrained_J_Regressor.pt')).numpy()
    assert J.shape == (17, 6890) and np.array_equal(J[J_np <= 0], J_np[J_np <= 0]) and (J[J_np > 0] != J_np[J_np > 0]).all()
    assert doc['support']['after'] == [int(c) for c in (J > 0).sum(1)]
    # the initial scores are those of the initial regressor on these meshes
    held = rf.holdout_split(N_CMD, 0.34, _paths(N_CMD))
    assert held.sum() == 32
    joints = np.einsum('jv,bvc->bjc', _normalised(J_np, None), verts.astype(np.float64))
    gt = gt.astype(np.float64)
    err = np.linalg.norm((joints - joints[:, :1]) - (gt - gt[:, :1]) / 1000, axis=2).mean(1) * 1000
    assert abs(err[~held].mean() - doc['initial']['train']['mpjpe_mm']) < 1e-2 and abs(err[held].mean() - doc['initial']['holdout']['mpjpe_mm']) < 1e-2


def test_the_evaluation_accepts_the_fitted_checkpoint(command_runs):
    outs, rep, J_np, verts, gt = command_runs
    assert sorted(os.listdir(rep)) == ['eval.json', 'eval.md']
    doc = _mod('eval_report').load(rep)
    assert doc['j_regressor_retrained']['path'].endswith('retrained_J_Regressor.pt')
