#!/usr/bin/env python3
"""Generate tests/golden/g13_eval_protocol.npz by IMPORTING the reference's own modules (as tests/golden/make_golden_eval.py does).

Run only in the build container (needs /root/reference):  python tests/golden/make_golden_protocol.py
The reference's Python never travels; only the small .npz written here is committed.

Inputs: the 48 poses of g11 (8 each of the six G11_FAMILIES of tests/eval_report_cases.py, regenerated from their seeds and compared
with what g11 stores).  Per mask of protocol_cases.G13_MASKS (lsp14, tri3, pair2) and per root (joint 0, the midpoint of the hips): the
reference's batch_compute_similarity_transform_torch in float32 on the centred, selected joints -- the (48,17) plain and aligned
per-joint errors, 0 in the excluded columns.  Each family's cap of eval_report_cases.FAMILIES is asserted on the float32-to-float64
distance of the aligned error: if a seed breaks a cap, another seed is picked, never a wider cap.
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
ref_constants = importlib.import_module('scripts.constants')

import eval_report_cases as ec  # noqa: E402
import protocol_cases as pc  # noqa: E402

# the reference's own list of the 14 joints
assert sorted(int(j) for j in ref_constants.H36M_TO_J14) == pc.joints_of(pc.MASKS['lsp14'])

preds, tgts = zip(*[ec.family_cases(name, ec.G11_POSES) for name in ec.G11_FAMILIES])
pred, tgt = np.concatenate(preds), np.concatenate(tgts)
g11 = np.load(os.path.join(HERE, 'g11_eval_degenerate.npz'))
assert np.array_equal(pred, g11['pred']) and np.array_equal(tgt, g11['target_mm'])

arrs = {}
for mask_name in pc.G13_MASKS:
    for root_name, root in pc.ROOTS.items():
        mask = pc.MASKS[mask_name]
        e32, pa32 = pc.evaluate_protocol(pred, tgt, mask, root, pc.TARGET_MM, torch.float32, ref_eval.batch_compute_similarity_transform_torch)
        # the restatement equals the reference bit for bit on these inputs
        r32 = pc.evaluate_protocol(pred, tgt, mask, root, pc.TARGET_MM, torch.float32)
        assert np.array_equal(r32[0], e32) and np.array_equal(r32[1], pa32, equal_nan=True)
        e64, pa64 = pc.evaluate_protocol(pred, tgt, mask, root, pc.TARGET_MM, torch.float64)
        assert np.isfinite(e32).all() and np.isfinite(pa32).all()
        for k, name in enumerate(ec.G11_FAMILIES):
            sl = slice(k * ec.G11_POSES, (k + 1) * ec.G11_POSES)
            d_plain, d_pa = pc.distance(e32[sl], e64[sl]), pc.distance(pa32[sl], pa64[sl])
            print(f'g13 {mask_name:6s} {root_name:6s} {name:20s}: reference fp32 against float64 plain {d_plain:.3e} m, PA {d_pa:.3e} m')
            assert d_pa <= ec.FAMILIES[name][1] and d_plain <= ec.FAMILIES[name][1], f'{name}: pick another seed'
        arrs[pc.g13_key(mask_name, root_name, 'err_j')] = e32
        arrs[pc.g13_key(mask_name, root_name, 'err_pa_j')] = pa32
path = os.path.join(HERE, 'g13_eval_protocol.npz')
np.savez_compressed(path, **arrs)
print('g13_eval_protocol.npz', {k: v.shape for k, v in arrs.items()}, os.path.getsize(path), 'bytes')
assert os.path.getsize(path) <= 64 * 1024
