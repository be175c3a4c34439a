#!/usr/bin/env python3
"""Device-event time of one moments pass over a table (jrr_jfit_moments) beside one epoch of Adam steps on the same table
(jrr_jfit_run) -- DESIGN.md, "The exact solve":

    python tools/exp/jmom_time.py [--rows 65536] [--batch 4096] [--reps 15] [--rings-ns 0] [--out profiles/jmom_time.json]

The table: `rows` synthetic samples with the shipped regressor's support (62 entries on 58 vertices), random vertices of body size and
ground truth -- neither time depends on the values.  HIP events around ONE jrr_jfit_moments call over all rows (two launches: the
chunks' partial tiles, then the slab sums) and around one epoch of jrr_jfit_run at `batch` (rows / batch steps, one C call, one launch
per step), alternating; two warm-up rounds of each, then `reps` timed rounds; the median and the spread (min, max), in microseconds.
Bytes of a pass are computed from the shapes: the cache rows, read once.  `--rings-ns N` adds a second table whose support is N
random vertices (what `--fit_rings 1` makes of the shipped support is about 380) and times the moments pass on it alone.  Needs a GPU:
it fails without one."""
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


def _table(eng, J, rows, dev, g):
    fit = eng.RegressorFit(J, None, rows)
    fit.cache[:, :3 * fit.ns] = (torch.randn(rows, 3 * fit.ns, generator=g) * 0.3).to(dev)
    gt = torch.randn(rows, NJ, 3, generator=g) * 300
    fit.cache[:, 3 * fit.ns:3 * fit.ns + 3 * NJ] = (gt - gt[:, :1]).reshape(rows, -1).to(dev)
    return fit


def _once(fn):
    """microseconds between two events around fn()"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=65536)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--rings-ns', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jmom_time.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('jmom_time.py measures on a GPU; none is visible')
    eng = importlib.import_module(PKG + '.engine')
    sm = importlib.import_module(PKG + '.smpl_model')
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    J = torch.from_numpy(sm.default_h36m_regressor()).float().to(dev)
    fit = _table(eng, J, a.rows, dev, g)
    steps = (a.rows + a.batch - 1) // a.batch
    loss = torch.zeros(steps, device=dev)
    times = {'moments': [], 'epoch': []}
    for rep in range(a.reps + 2):                                   # alternating, so that neither owns the caches
        for name, fn in (('moments', lambda: fit.moments(0, a.rows)), ('epoch', lambda: fit.run(a.batch, 0, steps, 1e-5, loss=loss))):
            t = _once(fn)
            if rep >= 2:
                times[name].append(t)
    med = {k: float(np.median(v)) for k, v in times.items()}
    nbytes = a.rows * fit.row_floats * 4
    W = fit.ns + NJ
    tiles = ((W + 15) // 16) * ((W + 15) // 16 + 1) // 2
    res = {'rows': a.rows, 'ns': fit.ns, 'entries': fit.entries, 'row_bytes': fit.row_floats * 4, 'reps': a.reps, 'batch': a.batch,
           'steps_per_epoch': steps, 'moments_us': med['moments'], 'moments_us_min_max': [min(times['moments']), max(times['moments'])],
           'epoch_us': med['epoch'], 'epoch_us_min_max': [min(times['epoch']), max(times['epoch'])], 'bytes_per_pass': nbytes,
           'moments_gbytes_per_s': nbytes / med['moments'] / 1e3, 'tiles': tiles,
           'mfma_per_pass': tiles * 3 * ((a.rows + 3) // 4), 'final_loss': float(loss[-1].item())}
    print(f'{a.rows} rows, NS {fit.ns} (W {W}, {tiles} tiles): moments pass {res["moments_us"]:.1f} us ({res["moments_us_min_max"][0]:.1f} .. '
          f'{res["moments_us_min_max"][1]:.1f}), {nbytes} bytes, {res["moments_gbytes_per_s"]:.0f} GB/s; one epoch of {steps} Adam steps at '
          f'batch {a.batch}: {res["epoch_us"]:.1f} us ({res["epoch_us_min_max"][0]:.1f} .. {res["epoch_us_min_max"][1]:.1f})')
    if a.rings_ns > 0:
        rng = np.random.RandomState(0)
        Jw = torch.zeros(NJ, NV)
        cols = torch.from_numpy(np.sort(rng.choice(NV, a.rings_ns, replace=False)))
        for k, c in enumerate(cols.tolist()):
            Jw[k % NJ, c] = 1.0
        wide = _table(eng, Jw.to(dev), a.rows, dev, g)
        t = [_once(lambda: wide.moments(0, a.rows)) for _ in range(a.reps + 2)][2:]
        Ww = wide.ns + NJ
        tw = ((Ww + 15) // 16) * ((Ww + 15) // 16 + 1) // 2
        res['wide'] = {'ns': wide.ns, 'tiles': tw, 'moments_us': float(np.median(t)), 'moments_us_min_max': [min(t), max(t)],
                       'bytes_per_pass': a.rows * wide.row_floats * 4, 'mfma_per_pass': tw * 3 * ((a.rows + 3) // 4)}
        print(f'NS {wide.ns} (W {Ww}, {tw} tiles): moments pass {res["wide"]["moments_us"]:.1f} us ({min(t):.1f} .. {max(t):.1f}), '
              f'{res["wide"]["bytes_per_pass"]} bytes')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
