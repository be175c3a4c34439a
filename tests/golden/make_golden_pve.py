#!/usr/bin/env python3
"""Generate tests/golden/g12_vertex_error.npz by IMPORTING the reference's own module (as tests/golden/make_golden_eval.py does).

Run only in the build container (needs /root/reference):  python tests/golden/make_golden_pve.py
The reference's Python never travels; only the small .npz written here is committed.  The meshes are regenerated from the seeds of
tests/vertex_error_cases.py and are not stored.

Per family of vertex_error_cases.FAMILIES and vertex count of G12_VERTS, G12_POSES poses: the reference's
batch_compute_similarity_transform_torch on the root-centred float32 meshes, then
  <family>_<n>_d, _e      (4, len(subset(n))) float32: the plain and the aligned per-vertex distance at the vertices subset(n)
  <family>_<n>_pve, _pa   (4,) float32: their means over ALL vertices (torch's float32 mean)
and, printed, the reference's own float32 distance from the same lines in float64 (oracle.batch_compute_similarity_transform_torch on
double inputs): the floor of the tests' bounds (vertex_error_cases.FLOOR_VERTEX, FLOOR_POSE) is its maximum rounded up to one digit.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'

sys.argv = ['x', '--device', 'cpu']
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
ref_eval = importlib.import_module('scripts.eval_utils')

import oracle  # noqa: E402
import vertex_error_cases as vc  # noqa: E402
T = torch.from_numpy

arrs, worst_v, worst_p = {}, 0.0, 0.0
for name in vc.FAMILIES:
    for n in vc.G12_VERTS:
        pred, gt, rp, rg = vc.family_case(name, n)
        x = T(pred) - T(rp)[:, None, :]
        y = T(gt) - T(rg)[:, None, :]
        hat = ref_eval.batch_compute_similarity_transform_torch(x, y)
        d = torch.sqrt(((x - y) ** 2).sum(dim=-1))
        e = torch.sqrt(((hat - y) ** 2).sum(dim=-1))
        assert torch.equal(oracle.batch_compute_similarity_transform_torch(x, y), hat)      # the port equals the reference bit for bit
        x64 = T(pred).double() - T(rp).double()[:, None, :]
        y64 = T(gt).double() - T(rg).double()[:, None, :]
        d64 = torch.sqrt(((x64 - y64) ** 2).sum(dim=-1))
        e64 = torch.sqrt(((oracle.batch_compute_similarity_transform_torch(x64, y64) - y64) ** 2).sum(dim=-1))
        dv = max((d.double() - d64).abs().max().item(), (e.double() - e64).abs().max().item())
        dp = max((d.mean(1).double() - d64.mean(1)).abs().max().item(), (e.mean(1).double() - e64.mean(1)).abs().max().item())
        assert np.isfinite(dv) and np.isfinite(dp), (name, n)
        print(f'g12 {name:16s} n_verts {n:5d}: reference fp32 against float64: per vertex {dv:.3e} m, per-pose means {dp:.3e} m')
        worst_v, worst_p = max(worst_v, dv), max(worst_p, dp)
        # the yardstick of the tests is the same float64 evaluation
        d_t, e_t, _, _ = vc.evaluate64(pred, gt, rp, rg)
        assert np.abs(d_t - d64.numpy()).max() <= 1e-12 and np.abs(e_t - e64.numpy()).max() <= 1e-9, (name, n)
        sub = vc.subset(n)
        arrs[f'{name}_{n}_d'], arrs[f'{name}_{n}_e'] = d.numpy()[:, sub], e.numpy()[:, sub]
        arrs[f'{name}_{n}_pve'], arrs[f'{name}_{n}_pa'] = d.mean(1).numpy(), e.mean(1).numpy()
print(f'maximum over the fixture: per vertex {worst_v:.3e} m, per-pose means {worst_p:.3e} m')
assert worst_v <= vc.FLOOR_VERTEX and worst_p <= vc.FLOOR_POSE, 'vertex_error_cases.FLOOR_* must be these maxima rounded up to one digit'
path = os.path.join(HERE, 'g12_vertex_error.npz')
np.savez_compressed(path, **arrs)
print('g12_vertex_error.npz', len(arrs), 'arrays', os.path.getsize(path), 'bytes')
assert os.path.getsize(path) <= 512 * 1024
