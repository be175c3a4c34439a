#!/usr/bin/env python3
"""Device-event time of one pricing pass (jrr_jfit_price) beside the torch float64 expression of the same sums -- DESIGN.md, "Every
vertex priced":

    python tools/exp/jprice_time.py [--batches 256 4096] [--reps 15] [--out profiles/jprice_time.json]

Random meshes of body size, the shipped regressor's support with uniform weights, NORM mode; neither time depends on the values.  HIP
events around ONE call of each, alternating in the same process; two warm-up rounds of each, then `reps` timed rounds; the median and
the spread (min, max), in microseconds.  The pass's time includes the upload of its lists (three small copies on the stream).  The torch
expression: the residuals by gathers in float64, then `einsum('bic,buc->iu', a, verts.double())` -- what a user without the kernel would
write; it reads the meshes once as fp32 and once more as the fp64 copy it makes.  The stream bound: the pass must read batch * 82 680
bytes of meshes once, at the 6.3 TB/s a streaming kernel reaches on this part.  Needs a GPU: it fails without one."""
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
NJ, NV = 17, 6890
HBM_BYTES_PER_S = 6.3e12


def _once(fn):
    """microseconds between two events around fn()"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1000.0


def _torch_sums(verts, gt, cands_dev, x_dev, delta):
    q = torch.stack([(x_dev[i][None, :, None] * verts[:, cands_dev[i]].double()).sum(1) for i in range(NJ)], 1)     # (B, 17, 3)
    r = q[:, 1:] - q[:, :1] - gt[:, 1:].double() / 1000.0
    a = r / torch.sqrt((r * r).sum(2, keepdim=True) + delta * delta)
    return torch.einsum('bic,buc->iu', a, verts.double())


def _measure(eng, batch, reps, dev, g, cands, x):
    verts = (torch.rand(batch, NV, 3, generator=g) * 2 - 1).mul(torch.tensor([0.35, 0.9, 0.15])).to(dev)
    gt = torch.randn(batch, NJ, 3, generator=g) * 300
    gt = (gt - gt[:, :1]).to(dev)
    cands_dev = [torch.from_numpy(c).to(dev) for c in cands]
    x_dev = [torch.from_numpy(w).to(dev) for w in x]
    out = torch.empty(eng.PRICE_DOUBLES, dtype=torch.float64, device=dev)
    fns = (('price', lambda: eng.price_vertices(verts, gt, cands, None, x, eng.PRICE_NORM, 1e-5, out=out)),
           ('torch', lambda: _torch_sums(verts, gt, cands_dev, x_dev, 1e-5)))
    times = {k: [] for k, _ in fns}
    for rep in range(reps + 2):                                      # alternating, so that neither owns the caches
        for name, fn in fns:
            t = _once(fn)
            if rep >= 2:
                times[name].append(t)
    S = out[:16 * NV].reshape(16, NV)
    ref = _torch_sums(verts, gt, cands_dev, x_dev, 1e-5)
    nbytes = batch * NV * 3 * 4
    res = {'batch': batch, 'reps': reps, 'bytes_of_meshes': nbytes, 'stream_bound_us': nbytes / HBM_BYTES_PER_S * 1e6,
           'mfma_per_pass': 431 * 3 * ((batch + 3) // 4), 'useful_fp64_flop_per_pass': 2 * 3 * batch * 16 * NV,
           'largest_distance_from_torch': float((S - ref).abs().max()), 'largest_sum': float(ref.abs().max())}
    for name, v in times.items():
        res[name + '_us'] = float(np.median(v))
        res[name + '_us_min_max'] = [min(v), max(v)]
    res['price_gbytes_per_s'] = nbytes / res['price_us'] / 1e3
    print(f'batch {batch}: price pass {res["price_us"]:.1f} us ({min(times["price"]):.1f} .. {max(times["price"]):.1f}), torch float64 '
          f'{res["torch_us"]:.1f} us ({min(times["torch"]):.1f} .. {max(times["torch"]):.1f}), stream bound {res["stream_bound_us"]:.1f} us '
          f'({nbytes} bytes, {res["price_gbytes_per_s"]:.0f} GB/s reached); distance from torch {res["largest_distance_from_torch"]:.2e}')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[256, 4096])
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jprice_time.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('jprice_time.py measures on a GPU; none is visible')
    eng = importlib.import_module(PKG + '.engine')
    sm = importlib.import_module(PKG + '.smpl_model')
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    J = sm.default_h36m_regressor()
    cands = [np.flatnonzero(J[i] > 0) for i in range(NJ)]
    x = [np.full(c.size, 1.0 / c.size) for c in cands]
    res = {str(b): _measure(eng, b, a.reps, dev, g, cands, x) for b in a.batches}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
