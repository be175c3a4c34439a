#!/usr/bin/env python3
"""Device-event times of jrr_vertex_error at 6890 vertices, batch 256 and 4096:

    python tools/vertex_error_time.py [--batches 256 4096] [--reps 30] [--out profiles/vertex_error_time.json]

Per batch: the launch as `--eval_pve` makes it (both tables, no per-pose or per-vertex rows), the launch with every output, the
launch with the per-pose means alone, each ALTERNATING with the torch expression of the same per-pose quantity on the same device
(root-centring, the plain distance, torch.linalg.svd of the batched 3x3 moment matrix, the det-sign fix, the aligned distance, both
means), and the stream bound: the bytes of both meshes read once over the HBM peak (8 TB/s).  The first call of each also checks
that the two agree to 1e-5 m.  At the largest batch the same at 7168 and 7169 vertices (`--paths`): the last size whose vertices a
workgroup keeps in registers, and the first whose second read comes from L2 / the memory-side cache.  Bytes are computed here from
the shapes.  Needs a GPU: it fails without one."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'joint-regressor-refinement_amd'
HBM_PEAK = 8.0e12            # bytes per second


def torch_pve(pred, gt, rp, rg):
    """(pve, pa_pve) (B,) of the torch-on-GPU expression: scripts/eval_utils.py:7-58 on all vertices, torch.linalg.svd"""
    x, y = pred - rp[:, None, :], gt - rg[:, None, :]
    pve = (x - y).norm(dim=-1).mean(1)
    mu1, mu2 = x.mean(1, keepdim=True), y.mean(1, keepdim=True)
    X1, X2 = x - mu1, y - mu2
    var1 = (X1 ** 2).sum((1, 2))
    K = X1.transpose(1, 2) @ X2
    U, _, Vh = torch.linalg.svd(K)
    V = Vh.transpose(1, 2)
    Z = torch.eye(3, device=x.device).repeat(x.shape[0], 1, 1)
    Z[:, 2, 2] = torch.sign(torch.det(U @ Vh))
    R = V @ Z @ U.transpose(1, 2)
    scale = (R @ K).diagonal(dim1=1, dim2=2).sum(1) / var1
    t = mu2.transpose(1, 2) - scale[:, None, None] * (R @ mu1.transpose(1, 2))
    hat = scale[:, None, None] * (x @ R.transpose(1, 2)) + t.transpose(1, 2)
    return pve, (hat - y).norm(dim=-1).mean(1)


def timed_pair(fn, other, reps):
    """median ms of fn and of other, alternating"""
    for _ in range(3):
        fn()
        other()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for a, b, c in ev:
        a.record()
        fn()
        b.record()
        other()
        c.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b, _ in ev])), float(np.median([b.elapsed_time(c) for _, b, c in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[256, 4096])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--paths', type=int, nargs='*', default=[7168, 7169],
                    help='vertex counts timed at the largest batch as well: the last one a workgroup keeps in registers and the first it reads again')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vertex_error_time.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('vertex_error_time.py measures on a GPU; none is visible')
    eng = importlib.import_module(PKG + '.engine')
    dev = torch.device('cuda:0')
    rows = {}
    for B, NV in [(B, 6890) for B in a.batches] + [(max(a.batches), v) for v in a.paths]:
        g = torch.Generator().manual_seed(B)
        gt = (torch.randn(B, NV, 3, generator=g) * torch.tensor([0.15, 0.5, 0.05])).to(dev)
        pred = (gt * 1.05 + torch.randn(B, NV, 3, generator=g).to(dev) * 0.02 + 0.1).contiguous()
        rp, rg = pred.mean(1).contiguous(), gt.mean(1).contiguous()
        group = (torch.arange(B, dtype=torch.int32) % 15).to(dev)
        part = (torch.arange(NV, dtype=torch.int32) * 24 // NV).to(dev)
        acc = torch.zeros(15 * eng.PVE_ACC_ROW + eng.PVE_ACC_TRAILER, dtype=torch.int64, device=dev)
        acc_v = torch.zeros(2, NV, dtype=torch.int64, device=dev)
        pve, pa, _, _ = eng.vertex_error(pred, gt, rp, rg, rows=False)
        t_pve, t_pa = torch_pve(pred, gt, rp, rg)
        agree = max(float((pve - t_pve).abs().max()), float((pa - t_pa).abs().max()))
        assert agree <= 1e-5, agree
        read = 2 * B * NV * 3 * 4
        bound_ms = read / HBM_PEAK * 1e3
        other = lambda: torch_pve(pred, gt, rp, rg)
        launches = {
            'report': (lambda: eng.vertex_error(pred, gt, rp, rg, group=group, n_groups=15, acc=acc, acc_v=acc_v, means=False, rows=False), read),
            'report_parts': (lambda: eng.vertex_error(pred, gt, rp, rg, group=group, part=part, n_parts=24, n_groups=15, acc=acc, acc_v=acc_v,
                                                      means=False, rows=False), read),
            'means': (lambda: eng.vertex_error(pred, gt, rp, rg, rows=False), read),
            'everything': (lambda: eng.vertex_error(pred, gt, rp, rg, group=group, n_groups=15, acc=acc, acc_v=acc_v), read + 2 * B * NV * 4),
        }
        for name, (fn, nbytes) in launches.items():
            ms, ms_torch = timed_pair(fn, other, a.reps)
            rows[f'{name}_b{B}' + ('' if NV == 6890 else f'_v{NV}')] = {'ms': ms, 'ms_torch': ms_torch, 'bytes': nbytes, 'GB_per_s': nbytes / ms / 1e6,
                                                                        'stream_bound_ms': bound_ms, 'agree_m': agree}
            print(f'B {B:5d} n_verts {NV:5d} {name:<14s} {ms:9.4f} ms   torch {ms_torch:9.4f} ms   stream bound {bound_ms:7.4f} ms   ({nbytes / ms / 1e6:8.1f} GB/s)')
    doc = {'n_verts': 6890, 'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'hbm_peak_bytes_per_s': HBM_PEAK, 'rows': rows,
           'note': 'median of device-event times, each launch alternating with the torch expression of the same per-pose quantity'}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
