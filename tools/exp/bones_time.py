#!/usr/bin/env python3
"""Device-event time of the bone report's two launches (jrr_bone_error + jrr_bone_accumulate) beside a torch expression of the same
per-pose values -- DESIGN.md section 3q:

    python tools/exp/bones_time.py [--batches 256 4096] [--reps 15] [--out profiles/bones_time.json]

Random skeletons of body size, the target a rotated, scaled, noisy copy; three groups; neither time depends on the values.  HIP events
around ONE call of each, alternating in the same process; two warm-up rounds of each, then `reps` timed rounds; the median and the spread
(min, max), in microseconds.  The torch expression is what a user without the kernel would write on the GPU: the bone vectors by index
arithmetic, `atan2` of cross and dot, the Procrustes rotation by `torch.linalg.svd` of the batched 3x3 moments, the two rebuilt
skeletons bone by bone along the chains, and per-group sums by `index_add_` -- float32 sums, so unlike the kernel's table neither exact
nor independent of order.  No threshold is set: the report launches the pair once per evaluation batch and regressor.  Needs a GPU: it
fails without one."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PKG = 'joint-regressor-refinement_amd'
NJ, N_GROUPS = 17, 3
PARENT = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)


def _once(fn):
    """microseconds between two events around fn()"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1000.0


def _angle(a, b):
    return torch.atan2(torch.linalg.cross(a, b).norm(dim=-1), (a * b).sum(-1))


def _torch_values(pred, gt_mm, child, parent):
    """(B,98): the layout of include/jrr.h, JRR_BONE_*"""
    x = pred - pred[:, :1]
    y = gt_mm / 1000
    y = y - y[:, :1]
    u, v = x[:, child] - x[:, parent], y[:, child] - y[:, parent]
    lp, lg = u.norm(dim=-1), v.norm(dim=-1)
    x1, x2 = x - x.mean(1, keepdim=True), y - y.mean(1, keepdim=True)
    K = x1.transpose(1, 2) @ x2
    U, _, Vh = torch.linalg.svd(K)
    V = Vh.transpose(1, 2)
    Z = torch.eye(3, device=pred.device).repeat(pred.shape[0], 1, 1)
    Z[:, 2, 2] = torch.sign(torch.linalg.det(U @ Vh))
    R = V @ Z @ U.transpose(1, 2)
    ru = u @ R.transpose(1, 2)
    xd, xl = [torch.zeros_like(x[:, 0])] * NJ, [torch.zeros_like(x[:, 0])] * NJ
    for b in range(1, NJ):
        xd[b] = xd[PARENT[b]] + u[:, b - 1] * (lg[:, b - 1] / lp[:, b - 1])[:, None]
        xl[b] = xl[PARENT[b]] + v[:, b - 1] * (lp[:, b - 1] / lg[:, b - 1])[:, None]
    e_dir, e_len = (torch.stack(xd, 1) - y).norm(dim=-1), (torch.stack(xl, 1) - y).norm(dim=-1)
    return torch.cat([lp, lg, _angle(u, v), _angle(ru, v), e_dir, e_len], 1)


def _torch_pair(pred, gt_mm, group, child, parent, sums):
    vals = _torch_values(pred, gt_mm, child, parent)
    sums.index_add_(0, group.long(), vals)
    return vals


def _measure(eng, batch, reps, dev, g):
    pred = (torch.randn(batch, NJ, 3, generator=g) * torch.tensor([0.15, 0.5, 0.05])).to(dev)
    q, _ = torch.linalg.qr(torch.randn(batch, 3, 3, generator=g))
    gt = ((pred.cpu() @ q) * 1.1 + 0.02 * torch.randn(batch, NJ, 3, generator=g) + 0.2).mul(1000).to(dev)
    group = torch.randint(0, N_GROUPS, (batch,), generator=g, dtype=torch.int32).to(dev)
    child, parent = torch.arange(1, NJ, device=dev), torch.tensor(PARENT[1:], device=dev)
    vals = torch.empty(batch, eng.BONE_VALS, device=dev)
    acc = torch.zeros(N_GROUPS * eng.BONE_ACC_ROW + eng.BONE_ACC_TRAILER, dtype=torch.int64, device=dev)
    sums = torch.zeros(N_GROUPS, eng.BONE_VALS, device=dev)

    def pair():
        eng.bone_error(pred, gt, out=vals)
        eng.bone_accumulate(vals, group, N_GROUPS, acc)

    fns = (('bones', pair), ('bone_error', lambda: eng.bone_error(pred, gt, out=vals)),
           ('bone_accumulate', lambda: eng.bone_accumulate(vals, group, N_GROUPS, acc)),
           ('torch', lambda: _torch_pair(pred, gt, group, child, parent, sums)))
    times = {k: [] for k, _ in fns}
    for rep in range(reps + 2):                                      # alternating, so that none owns the caches
        for name, fn in fns:
            t = _once(fn)
            if rep >= 2:
                times[name].append(t)
    ref = _torch_values(pred, gt, child, parent)
    res = {'batch': batch, 'reps': reps, 'groups': N_GROUPS, 'bytes_in': batch * NJ * 3 * 4 * 2, 'bytes_out': batch * eng.BONE_VALS * 4,
           'largest_distance_from_torch': float((vals - ref).abs().max())}
    for name, v in times.items():
        res[name + '_us'] = float(np.median(v))
        res[name + '_us_min_max'] = [min(v), max(v)]
    print(f'batch {batch}: bone_error + bone_accumulate {res["bones_us"]:.1f} us ({min(times["bones"]):.1f} .. {max(times["bones"]):.1f}) = '
          f'{res["bone_error_us"]:.1f} + {res["bone_accumulate_us"]:.1f} alone; torch {res["torch_us"]:.1f} us ({min(times["torch"]):.1f} .. '
          f'{max(times["torch"]):.1f}); distance from torch {res["largest_distance_from_torch"]:.2e}')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[256, 4096])
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bones_time.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bones_time.py measures on a GPU; none is visible')
    eng = importlib.import_module(PKG + '.engine')
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    res = {str(b): _measure(eng, b, a.reps, dev, g) for b in a.batches}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
